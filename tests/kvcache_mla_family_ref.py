"""ONE float64 restatement of the thirteen MLA latent-cache calls (ffpa_attn_amd/kvcache.py: the dense, ragged, FP8, tree-mask, sparse, 656-byte-row and cascade
calls), written from their docstrings and from nothing in the kernels, and the seeded case generator of the family sweep — ``draw_case`` / ``materialize`` /
``reference`` in the vocabulary of tests/kvcache_ref.py.  Every call is the same three steps: each sequence (each token, for the sparse calls) has a logical list
of latent rows — taken after the append where there is one, dequantised where the pool is quantised —, a boolean visibility ``[query token, key]`` made from the
case's Python values alone (bottom-right causal, the tree mask over the last rows, the first ``count`` entries of an index list, or everything), and a float64
softmax in the operations and order of ``kvcache_ref.attend``.  ``reference`` returns the tuple ``kvcache_ref.check`` takes — one row per query token —, the
visible-value statistics its allowance wants and the pool's expected storage after the append.  Plain torch + numpy (any device): tested without a GPU
(tests/test_kvcache_mla_family.py) and used by tests/test_kvcache_mla_family_gpu.py.  The quantisers (``quantize_latent_rows``, ``pack_latent_rows_ds``,
``unpack_latent_rows_ds``) are the library's plain-torch DEFINITIONS of its formats, not kernels."""

from __future__ import annotations

import random

import torch

import kvcache_mla_cases as MC
import kvcache_ref as R
import model_values as mv
import tree_ref

D, DV, DS_ROW = 576, 512, 656
SCALE = 192 ** -0.5
F8 = torch.float8_e4m3fn
INT_MAX, INT_MIN = 2 ** 31 - 1, -(2 ** 31)

CALLS = (
  "ffpa_attn_with_kvcache_mla",
  "ffpa_attn_varlen_with_kvcache_mla",
  "ffpa_attn_with_kvcache_mla_fp8",
  "ffpa_attn_varlen_with_kvcache_mla_fp8",
  "ffpa_attn_with_kvcache_mla_tree",
  "ffpa_attn_varlen_with_kvcache_mla_tree",
  "ffpa_attn_with_kvcache_mla_tree_fp8",
  "ffpa_attn_varlen_with_kvcache_mla_tree_fp8",
  "ffpa_attn_with_kvcache_mla_sparse",
  "ffpa_attn_with_kvcache_mla_sparse_fp8",
  "ffpa_attn_with_kvcache_mla_sparse_ds",
  "ffpa_attn_with_kvcache_mla_cascade",
  "ffpa_attn_with_kvcache_mla_cascade_fp8",
)
HEADS = ((1, 1), (8, 1), (16, 1), (24, 1), (64, 1), (80, 1), (128, 1), (32, 2), (16, 2), (6, 3))
UNIFORM_SQ = (1, 2, 3, 5, 8)
TREE_SQ = (1, 2, 64, 5, 17, 33, 8, 63)
PAGES = (64, 128, 256, 0)  # 0: a contiguous cache
SPARSE_FORMS = ("flat", "page1", "page16", "page64", "padded")
SPARSE_PAGE = {"flat": 0, "page1": 1, "page16": 16, "page64": 64, "padded": 0}
SPLITS = R.SPLITS
STREAMS = R.STREAMS
APPENDS = ("none", "same", "few", "edge")
KV_SCALES = (0.25, 1.0, 0.37)
BEHIND = (-1, INT_MIN, INT_MAX, 2 ** 30)  # what sits behind a count: never turned into an address
SWEEP_SEEDS = tuple(range(104))
# the model_values families a case may take: every one of tests/kvcache_mla_cases.py over a 16-bit pool; over a quantised pool and under the cascade (whose
# sequences share their first rows) the ones whose property does not hang on exact small integers in a column or on the pairing of q and k by sequence
MODEL_ANY = MC.MODEL_VARIANTS
MODEL_ROBUST = ("outliers", "large_logits")


def traits(call: str) -> dict:
  return {"ragged": "_varlen_" in call, "tree": "_tree" in call, "sparse": "_sparse" in call, "ds": call.endswith("_ds"), "fp8": call.endswith("_fp8"),
          "cascade": "_cascade" in call}


def kernel_of(c: dict) -> str:
  """What the plan's kernel name of a case's attention launches starts with."""
  kind = ("_sparse" if c["sparse"] else "") + ("_tree" if c["tree"] else "") + ("_fp8" if c["fp8"] else "") + ("_ds" if c["ds"] else "")
  return f"ffpa_fwd_m16_mla{kind}_kernel<{c['dtype']}, 576, dv=512"


# ----------------------------------------------------------------------------- the sweep's cases
def draw_case(seed: int) -> dict:
  """The family sweep's case of a seed: plain Python values only.  The call is ``CALLS[seed % 13]``; with ``k = seed // 13`` the axes a call must meet (split
  counts, pages / pool forms, append kinds) walk their values once per four (five) k, the others are cycled with co-prime strides (``kvcache_ref._cycle``);
  lengths, token counts, index lists and the data come from the seed's own generator."""
  rng = random.Random(seed * 7919 + 31)
  ci, k = seed % len(CALLS), seed // len(CALLS)
  call = CALLS[ci]
  c = {"seed": seed, "call": call, **traits(call)}
  c["dtype"] = "bf16" if c["ds"] else ("bf16", "fp16")[R._cycle(seed, 2)]
  c["heads"] = HEADS[R._cycle(seed, 10, 3)]
  c["num_splits"] = SPLITS[(k + ci) % 4]
  c["stream"] = STREAMS[R._cycle(seed, 3)]
  c["causal"] = False if c["tree"] or c["sparse"] else bool(R._cycle(seed, 2, 1, 1))
  c["kv_scale"] = KV_SCALES[R._cycle(seed, 3, 1, 2)] if c["fp8"] else None
  c["table_layout"] = R.TABLE_LAYOUTS[R._cycle(seed, 3, 2, 1)]
  c["lens_strided"] = bool((seed // 3) % 2)
  c["pad"] = 16 if seed % 3 == 0 else 0  # columns of layout padding behind every row (bytes, for the byte pools)
  c["model"] = None
  if seed % 4 == 1:
    names = MODEL_ROBUST if c["fp8"] or c["ds"] or c["cascade"] else MODEL_ANY
    c["model"] = names[(seed // 4) % len(names)]
    if c["heads"][0] < 16:  # (a family shows its property on a few dozen rows at least: tests/kvcache_mla_cases.py takes 16 and 32 heads)
      c["heads"] = ((16, 1), (32, 2))[(seed // 4) % 2]
  c["scale"] = MC.MODEL_SCALE if c["model"] else SCALE
  c["long"] = (seed % 5 == 3 and not c["model"]) or seed % 20 == 14  # one seed in five (13, 33, ... take a model family: their neighbour is long instead)
  (_draw_sparse if c["sparse"] else _draw_dense)(c, rng, k, ci)
  return c


def _draw_dense(c: dict, rng, k: int, ci: int) -> None:
  hq, hkv = c["heads"]
  model, long_ = c["model"], c["long"]
  c["page"] = page = PAGES[:3][(k + ci) % 3] if c["cascade"] else PAGES[(k + 2 * ci + ci // 4) % 4]
  unit = page or 64
  B = 1 + R._cycle(c["seed"], 5, 2, 1)
  if c["ragged"] or c["cascade"]:
    B = max(B, 3)
  if model:
    B = MC.MODEL_BATCH
  c["B"] = B
  # tokens per sequence
  sq = TREE_SQ[k] if c["tree"] else UNIFORM_SQ[R._cycle(c["seed"], 5, 2)]
  if c["tree"] and (model or long_):
    sq = (3, 8)[k % 2]
  if c["ragged"] and not model:
    big = lambda: rng.randrange(40, 65 if c["tree"] else 71)
    qlens = [rng.choice((0, 1, 1, 2, 3, 5, big())) for _ in range(B)]
    first = [0, 1, big()]
    rng.shuffle(first)
    qlens[:3] = first
  else:
    qlens = [sq] * B
  c["qlens"], c["Sq"] = qlens, (max(qlens) if c["ragged"] else sq)
  L = MC.MODEL_LENS[k % 2] if model else 0
  reach = L + 10 if model else rng.randrange(2500, 6000) if long_ else rng.randrange(100, 1400)
  c["pages_per_seq"] = pps = -(-reach // unit) + 1
  c["capacity"] = cap = pps * unit
  # the append
  mode = APPENDS[(k + 3 * ci) % 4]
  if mode == "none":
    snew = [None] * B
  elif c["ragged"]:
    snew = list(qlens)
  else:
    snew = [(1, 3)[(k // 4) % 2] if mode == "few" else sq] * B
  c["append"], c["snew"] = mode, snew
  new = [n or 0 for n in snew]
  # the lengths before the append
  edges = (0, -3, 1, 31, 32, 33, unit - 1, unit + 1, cap, cap + 5)
  if model:
    lens = [L - n for n in new]
  elif c["cascade"]:
    lens = None
  else:
    lens = [rng.choice(edges) if rng.random() < 0.3 else rng.randrange(1, cap) for _ in range(B)]
    if long_:
      lens[next(b for b in range(B) if 1 <= qlens[b] <= 8)] = rng.randrange(2500, cap)
      for b in range(B):
        if qlens[b] > 8:  # (the long cases keep to a handful of tokens: a chunk of 40 ... 70 tokens reads a short sequence)
          lens[b] = min(lens[b], rng.randrange(100, 1400))
    if all(n <= 0 for n in lens):
      lens[rng.randrange(B)] = rng.randrange(1, cap)
  # groups and shared prefixes (one sequence per group and nothing shared: every call but the cascade)
  sizes, share, stated = [1] * B, [0] * B, None
  if c["cascade"]:
    sizes = [B] if k % 2 == 0 else [max(1, B // 2), 0, B - max(1, B // 2)]
    c["prefix_on_device"] = on_device = (k // 2) % 2 == 1
    top = max(1, (L // 2 if model else cap // 3) // page)
    one = page * (top if model else rng.randrange(1, top + 1))
    share = [0 if n == 0 else one if not on_device or rng.random() < 0.5 else max(page, one - page) for n in sizes]
    half = page // 2 if rng.random() < 0.5 else 0  # (no page multiple: rounded down)
    stated = [s + half for s in share] if on_device else one + half
    if not model:
      lens, b = [], 0
      for g, n in enumerate(sizes):
        for _ in range(n):
          room = cap - share[g] - new[b] - 1
          lens.append(share[g] + (rng.choice((0, 1, sq, 70, 129)) if rng.random() < 0.5 else rng.randrange(0, room)) if room > 129 else share[g])
          b += 1
      if long_:
        lens[0] = max(lens[0], rng.randrange(2500, cap - new[0]))
      if mode == "none" and k >= 4:  # the stated prefix is longer than what one sequence holds: its pages are the shared ones, it holds fewer keys
        b = 1 if sizes[0] > 1 else sum(sizes[:2]) + 1
        lens[b] = share[0 if sizes[0] > 1 else 2] - rng.randrange(1, page)
  c["group_sizes"], c["share"], c["stated_prefix"] = sizes, share, stated
  if mode == "edge" and not model:
    live = [b for b in range(B) if new[b] > 0]
    if live:
      lens[rng.choice(live)] = cap - 1  # (the first new row fills the cache's last one, the others are dropped)
  c["lens"] = lens
  c["bad_unused_ids"] = bool(page) and rng.random() < 0.5
  if c["tree"]:
    c["mask_kind"] = ("tril", "ones")[k % 2] if model else tree_ref.MASK_KINDS[(k + ci) % 5]
    c["per_sequence"] = k % 2 == 1 and not model


def _draw_sparse(c: dict, rng, k: int, ci: int) -> None:
  model, long_ = c["model"], c["long"]
  c["form"] = form = SPARSE_FORMS[(k + ci) % 5]
  c["page"] = page = SPARSE_PAGE[form]
  sq = UNIFORM_SQ[R._cycle(c["seed"], 5, 2)]
  c["B"] = B = MC.MODEL_BATCH if model else 1 + k % 2
  c["Sq"], c["qlens"] = 1, [1] * (B * sq)
  c["T"] = T = B * sq
  c["append"] = "store" if c["ds"] and k % 2 == 1 else "none"
  if model:
    L = MC.MODEL_LENS[k % 2]
    c["topk"] = topk = L + 7
    c["counts"], c["counts_none"] = [L] * T, False
    c["num_rows"] = num_rows = -(-(B * L + 64) // 64) * 64
    c["model_tokens"] = (B, sq, L)
    slots = list(range(num_rows))
    rng.shuffle(slots)
    c["model_slots"] = [slots[b * L:(b + 1) * L] for b in range(B)]  # where the rows of sequence b lie; its tokens list them in order
    fill = lambda t, j: BEHIND[(t + j) % 4]
    c["indices"] = [c["model_slots"][t // sq] + [fill(t, j) for j in range(7)] for t in range(T)]
  else:
    c["topk"] = topk = rng.randrange(2500, 6000) if long_ else rng.choice((1, 33, 64)) if k == 0 else rng.randrange(100, 1400)
    edges = (0, -3, 1, 31, 32, 33, 63, 65, topk, topk + 5)
    c["counts_none"] = k % 4 == 2
    c["counts"] = [topk] * T if c["counts_none"] else [rng.choice(edges) if rng.random() < 0.3 else rng.randrange(1, topk + 1) for _ in range(T)]
    if long_ or all(n <= 0 for n in c["counts"]):
      c["counts"][rng.randrange(T)] = topk
    c["num_rows"] = num_rows = -(-(topk * 5 // 4 + 64) // 64) * 64
    rows = []
    for t in range(T):
      n = min(max(c["counts"][t], 0), topk)
      row = [rng.randrange(num_rows) for _ in range(n)]
      for j in range(1, n, max(1, n // 3)):  # duplicates in front of the count: a row named twice counts twice
        row[j] = row[j - 1]
      rows.append(row + [BEHIND[(t + j) % 4] for j in range(topk - n)])
    c["indices"] = rows
  c["capacity"] = topk
  if c["append"] == "store":  # a quarter of the rows some token names are written by store_latent_rows_ds in front of the call; two slots write nothing
    named = sorted({s for t in range(T) for s in c["indices"][t][:min(max(c["counts"][t], 0), topk)]})
    c["store_slots"] = [s for i, s in enumerate(named) if i % 4 == 0][:96] + [-1, num_rows + 3]
    rng.shuffle(c["store_slots"])


def counts_of(c: dict) -> list:
  """Sparse: the entries every token attends to, clamp(count, 0, topk)."""
  return [min(max(n, 0), c["topk"]) for n in c["counts"]]


def effective_lens(c: dict) -> list:
  """Dense: the keys every sequence attends over — clamp(len, 0, capacity), after the append where there is one."""
  cap = c["capacity"]
  return [min(max(n, 0) + (s or 0), cap) for n, s in zip(c["lens"], c["snew"])]


def case_mask(c: dict) -> torch.Tensor:
  """The tree mask of a drawn case (CPU): ``[W, W]`` or, per sequence, ``[B, W, W]``, W the largest token count (sequence b uses its top-left corner)."""
  rng = random.Random(c["seed"] * 977 + 5)
  W = max(c["Sq"], 1)
  if c["per_sequence"]:
    return torch.stack([tree_ref.draw_mask(c["mask_kind"], W, rng) for _ in range(c["B"])])
  return tree_ref.draw_mask(c["mask_kind"], W, rng)


def visibility(c: dict, b: int, device="cpu", mask=None) -> torch.Tensor:
  """``[tokens of b, keys of b]`` bool from the case's Python values alone: sequence b of a dense case (causal bottom-right, the tree mask over its last rows, or
  everything), token b of a sparse one (the first ``count`` entries of its list)."""
  if c["sparse"]:
    return torch.ones((1, counts_of(c)[b]), dtype=torch.bool, device=device)
  n, sq = effective_lens(c)[b], c["qlens"][b]
  if c["tree"]:
    m = case_mask(c) if mask is None else mask
    m = (m if m.dim() == 2 else m[b])[:sq, :sq]
    return tree_ref.visible(m, 0, n, sq, device) if sq else torch.ones((0, n), dtype=torch.bool, device=device)
  if c["causal"]:
    i, j = torch.arange(sq, device=device)[:, None], torch.arange(n, device=device)[None, :]
    return j <= i + (n - sq)
  return torch.ones((sq, n), dtype=torch.bool, device=device)


def visible_rows(c: dict) -> tuple:
  """``(query rows that see at least one key, query rows)`` per query head of a case."""
  units = range(c["T"] if c["sparse"] else c["B"])
  mask = case_mask(c) if c["tree"] else None
  seen = sum(int(visibility(c, b, mask=mask).any(dim=1).sum()) for b in units)
  return seen, sum(c["qlens"])


def row_classes(c: dict) -> set:
  """The classes the rows of a (sequence, latent head) — Hq / Hkv x tokens — of a case fall into."""
  group = c["heads"][0] // c["heads"][1]
  name = lambda r: "<16" if r < 16 else "16-63" if r < 64 else "64" if r == 64 else "65-127" if r < 128 else ">=128"
  return {name(group * n) for n in c["qlens"] if n > 0}


# ----------------------------------------------------------------------------- the tensors
def _quantisers():
  from ffpa_attn_amd.kvcache import pack_latent_rows_ds, quantize_latent_rows, unpack_latent_rows_ds

  return quantize_latent_rows, pack_latent_rows_ds, unpack_latent_rows_ds


def encode(c: dict, rows: torch.Tensor) -> torch.Tensor:
  """Latent rows ``[..., 576]`` in the pool's storage format: themselves (16 bits), ``quantize_latent_rows`` as bytes (FP8), ``pack_latent_rows_ds`` (656 bytes)."""
  quantize, pack, _ = _quantisers()
  if c["ds"]:
    return pack(rows)
  return quantize(rows, c["kv_scale"]).view(torch.uint8) if c["fp8"] else rows


def decode(c: dict, stored: torch.Tensor) -> torch.Tensor:
  """Stored rows -> the float64 values the call computes on: the FP8 suites' ``pool.double() * kv_scale``, ``unpack_latent_rows_ds`` of the 656-byte rows."""
  if c["ds"]:
    return _quantisers()[2](stored).double()
  return stored.contiguous().view(F8).double() * c["kv_scale"] if c["fp8"] else stored.double()


def _model_data(c: dict, shape):
  """``(q [B, Hq, Sq, D], k [B, Hkv, L, D])`` of the case's model_values family, as tests/kvcache_mla_cases.py ``build_model_case`` lays it out."""
  family, knobs, _ = mv.VARIANTS[c["model"]]
  case = {"variant": c["model"], "family": family, "knobs": dict(knobs), "shape": shape, "dtype": R.TORCH_DTYPE[c["dtype"]], "seed": 3000 + c["seed"]}
  q, k = MC.build_model_case(case)
  if c["cascade"]:
    k = k[:1].expand_as(k).contiguous()  # (the sequences of a cascade share their first rows: every sequence holds sequence 0's)
  return q, k


def _table(c: dict, g) -> "tuple[torch.Tensor, int]":
  """The block table of a paged dense case -> ``(table [B, pps], num_pages)``: shuffled ids; the sequences of a group share the ids of its shared pages."""
  B, pps, page = c["B"], c["pages_per_seq"], c["page"]
  shared = [s // page for s in c["share"]]
  total = sum(sp + n * (pps - sp) for sp, n in zip(shared, c["group_sizes"]))
  n_pages = total + 3
  ids = torch.randperm(n_pages, generator=g).tolist()
  table = torch.empty((B, pps), dtype=torch.int32)
  nxt = b = 0
  for sp, n in zip(shared, c["group_sizes"]):
    common = ids[nxt:nxt + sp]
    nxt += sp
    for _ in range(n):
      table[b] = torch.tensor(common + ids[nxt:nxt + pps - sp], dtype=torch.int32)
      nxt += pps - sp
      b += 1
  return table, n_pages


def _page_of(table, b: int, pos: torch.Tensor, page: int, n_pages: int) -> torch.Tensor:
  """The page (slab) that holds positions ``pos`` of sequence b: ``clamp(table[b, pos // page], 0, num_pages - 1)``; a contiguous cache: slab b."""
  if table is None:
    return torch.full_like(pos, b)
  return table[b].to(torch.int64)[pos // page].clamp(0, n_pages - 1)


def materialize(c: dict, device="cpu") -> dict:
  """The tensors of a drawn case on ``device`` in its layouts: ``q``, the pool ``kv_cache`` (a view of ``storage``, which owns its memory: one guard page / row on
  either side and ``pad`` columns behind every row), ``kv`` (the rows the call appends) or ``store_kv`` / ``store_slots`` (656-byte rows: written by slot in front of
  the call), and what the call takes of lengths, tables, masks, index lists and groups.  EVERY byte of the storage that no sequence reads before the append is
  NaN (0xFF in the byte pools): unused pages, rows behind a length, guard rows, padding."""
  dev = torch.device(device)
  g = torch.Generator().manual_seed(c["seed"] + 1000)
  gd = torch.Generator(device=dev).manual_seed(c["seed"] + 1000)
  dtype = R.TORCH_DTYPE[c["dtype"]]
  rnd = lambda *shape: torch.randn(shape, generator=gd, device=dev, dtype=torch.float32 if dev.type == "cpu" else dtype).to(dtype)
  hq, hkv = c["heads"]
  byte_pool = c["fp8"] or c["ds"]
  width = DS_ROW if c["ds"] else D
  new_storage = lambda *shape: (torch.full(shape, 0xFF, dtype=torch.uint8, device=dev) if byte_pool else torch.full(shape, float("nan"), dtype=dtype, device=dev))
  t = {"kv": None, "table": None}
  if c["sparse"]:
    T, num_rows, page = c["T"], c["num_rows"], c["page"]
    if c["model"]:
      B, sq, L = c["model_tokens"]
      qm, km = _model_data(c, (B, hq, hkv, sq, L, D))
      q = qm.permute(0, 2, 1, 3).reshape(T, hq, D).to(dev)
      rows = torch.zeros((num_rows, hkv, D), dtype=dtype)
      for b in range(B):
        rows[c["model_slots"][b]] = km[b].transpose(0, 1)
      rows = rows.to(dev)
    else:
      q, rows = rnd(T, hq, D), rnd(num_rows, hkv, D)
    named = torch.zeros(num_rows, dtype=torch.bool)
    for tkn, n in enumerate(counts_of(c)):
      if n:
        named[c["indices"][tkn][:n]] = True
    stored = encode(c, rows)
    if c["append"] == "store":
      slots = c["store_slots"]
      t["store_slots"] = torch.tensor(slots, dtype=torch.int32, device=dev)
      t["store_kv"] = rows[[min(max(s, 0), num_rows - 1) for s in slots]].contiguous()
      named[[s for s in slots if 0 <= s < num_rows]] = False  # (NaN until the store has written them)
    storage = new_storage(num_rows + 2, hkv, width + (48 if c["form"] == "padded" else c["pad"]))
    view = storage[1:-1, :, :width]
    view[named.to(dev)] = stored[named.to(dev)]
    if page:
      view = view.unflatten(0, (num_rows // page, page))
    t.update(q=q, storage=storage, view=view, kv_cache=view.view(F8) if c["fp8"] else view,
             indices=torch.tensor(c["indices"], dtype=torch.int32, device=dev),
             topk_lens=None if c["counts_none"] else R.lay_out_lens(torch.tensor(c["counts"], dtype=torch.int32, device=dev), c["lens_strided"]))
    return t
  # ---- the dense calls
  B, page, pps, cap, qlens = c["B"], c["page"], c["pages_per_seq"], c["capacity"], c["qlens"]
  T = sum(qlens)
  if page:
    table, n_pages = _table(c, g)
  else:
    table, n_pages, page = None, B, cap
  held = [min(max(n, 0), cap) for n in c["lens"]]
  if c["model"]:
    sq = c["Sq"]
    qm, km = _model_data(c, (B, hq, hkv, sq, MC.MODEL_LENS[(c["seed"] // len(CALLS)) % 2], D))
    q = qm.permute(0, 2, 1, 3).contiguous().to(dev)  # [B, Sq, Hq, D]
    km = km.permute(0, 2, 1, 3).to(dev)              # [B, L, Hkv, D]
    data = torch.zeros((n_pages, page, hkv, D), dtype=dtype, device=dev)
    for b in range(B):
      pos = torch.arange(held[b], device=dev)
      data[_page_of(None if table is None else table.to(dev), b, pos, page, n_pages), pos % page] = km[b, :held[b]]
    if c["snew"][0] is not None:
      t["kv"] = torch.stack([km[b, held[b]:held[b] + c["snew"][b]] for b in range(B)]).contiguous()
    if c["ragged"]:
      q = q.reshape(T, hq, D)
      t["kv"] = None if t["kv"] is None else t["kv"].reshape(T, hkv, D)
  else:
    q = rnd(T, hq, D) if c["ragged"] else rnd(B, c["Sq"], hq, D)
    data = rnd(n_pages, page, hkv, D)
    if c["snew"][0] is not None:
      t["kv"] = rnd(T, hkv, D) if c["ragged"] else rnd(B, c["snew"][0], hkv, D)
  used = torch.zeros((n_pages, page), dtype=torch.bool)
  for b in range(B):
    pos = torch.arange(held[b])
    used[_page_of(table, b, pos, page, n_pages), pos % page] = True
  storage = new_storage(n_pages + 2, page, hkv, D + c["pad"])
  view = storage[1:-1, :, :, :D]
  used = used.to(dev)
  view[used] = encode(c, data[used])
  if table is not None:
    eff = effective_lens(c)
    if c["bad_unused_ids"]:  # ids outside the pool behind every sequence's last used page (and behind the shared ones): never read
      b = 0
      for share, n in zip(c["share"], c["group_sizes"]):
        for _ in range(n):
          for j in range(max(-(-max(eff[b], held[b]) // page), share // page), pps):
            table[b, j] = (-1, n_pages, INT_MAX, INT_MIN)[(b + j) % 4]
          b += 1
    table = R.lay_out_table(table.to(dev), c["table_layout"])
  cu = [0]
  for n in qlens:
    cu.append(cu[-1] + n)
  t.update(q=q, storage=storage, view=view, kv_cache=view.view(F8) if c["fp8"] else view, table=table,
           lens=R.lay_out_lens(torch.tensor(c["lens"], dtype=torch.int32, device=dev), c["lens_strided"]),
           cu_seqlens_q=torch.tensor(cu, dtype=torch.int32, device=dev))
  if c["tree"]:
    t["tree_mask"] = case_mask(c).to(dev)
  if c["cascade"]:
    sizes = c["group_sizes"]
    bounds = [sum(sizes[:i]) for i in range(len(sizes) + 1)]
    t["cu_group_seqs"] = torch.tensor(bounds, dtype=torch.int32, device=dev) if len(sizes) > 1 else None
    t["max_group_seqs"] = max(sizes)
    t["shared_prefix_len"] = torch.tensor(c["stated_prefix"], dtype=torch.int32, device=dev) if c["prefix_on_device"] else c["stated_prefix"]
  return t


# ----------------------------------------------------------------------------- the calls, restated
def units(c: dict, t: dict):
  """-> ``(units, storage)``: per sequence (per token, for the sparse calls) ``(q [tokens, Hq, D], logical rows [n, Hkv, D] float64, visibility [tokens, n])``, and
  the pool's expected storage after the append — a clone of ``t["storage"]`` with the new rows written where the docstrings say, in the pool's format."""
  dev = t["q"].device
  storage = t["storage"].clone()
  view = R.reviewed(t["view"], t["storage"], storage)
  out = []
  if c["sparse"]:
    flat = view.flatten(0, 1) if view.dim() == 4 else view
    if c["append"] == "store":
      for i, s in enumerate(c["store_slots"]):
        if 0 <= s < c["num_rows"]:
          flat[s] = encode(c, t["store_kv"][i])
    for tkn, n in enumerate(counts_of(c)):
      slots = torch.tensor(c["indices"][tkn][:n], dtype=torch.int64, device=dev)
      out.append((t["q"][tkn:tkn + 1], decode(c, flat[slots]), visibility(c, tkn, dev)))
    return out, storage
  page, cap, n_pages, table = view.size(1), c["capacity"], view.size(0), t["table"]
  mask = t["tree_mask"] if c["tree"] else None
  start = 0
  for b, (n_tok, L) in enumerate(zip(c["qlens"], effective_lens(c))):
    snew = c["snew"][b]
    if snew:
      base = max(c["lens"][b], 0)
      pos = torch.arange(min(base, cap), min(base + snew, cap), device=dev)  # (rows at or past the capacity are dropped)
      new = t["kv"][start:start + snew] if c["ragged"] else t["kv"][b]
      if pos.numel():
        view[_page_of(table, b, pos, page, n_pages), pos % page] = encode(c, new[:pos.numel()])
    q = t["q"][start:start + n_tok] if c["ragged"] else t["q"][b]
    pos = torch.arange(L, device=dev)
    out.append((q, decode(c, view[_page_of(table, b, pos, page, n_pages), pos % page]), visibility(c, b, dev, mask)))
    start += n_tok
  return out, storage


def attend_units(us, scale: float, dv: int = DV):
  """``kvcache_ref.attend``'s float64 softmax — the same operations in the same order — over units of (q, rows, visibility): keys a row's ``D`` columns, values
  its first ``dv`` -> ``(check's tuple with one row per query token: o [T, 1, Hq, dv], lse [T, Hq, 1], pmax, p2sum; (largest |v|, RMS of v) over the rows the
  units hold)``."""
  T = sum(q.size(0) for q, _, _ in us)
  hq, dev = us[0][0].size(1), us[0][0].device
  o = torch.zeros((T, 1, hq, dv), dtype=torch.float64, device=dev)
  lse = torch.full((T, hq, 1), float("-inf"), dtype=torch.float64, device=dev)
  pmax = torch.zeros((T, hq, 1), dtype=torch.float64, device=dev)
  p2sum = torch.zeros((T, hq, 1), dtype=torch.float64, device=dev)
  amax, sumsq, cnt, start = 0.0, 0.0, 0, 0
  for q, rows, vis in us:
    sq, n = q.size(0), rows.size(0)
    if n:
      vals = rows[..., :dv]
      amax, sumsq, cnt = max(amax, float(vals.abs().max())), sumsq + float(vals.pow(2).sum()), cnt + vals.numel()
    if n == 0 or sq == 0:
      start += sq
      continue
    hkv, d = rows.size(1), rows.size(2)
    group = hq // hkv
    kb = rows.transpose(0, 1)                                                    # [Hkv, n, D]
    qb = q.double().transpose(0, 1).reshape(hkv, group * sq, d)                 # rows (head in group, token)
    s = torch.matmul(qb, kb.transpose(1, 2)) * scale
    s = s.masked_fill(~vis.repeat(group, 1)[None], float("-inf"))
    m = s.amax(dim=-1, keepdim=True)
    live = torch.isfinite(m)
    e = torch.exp(s - torch.where(live, m, torch.zeros_like(m)))
    l = e.sum(dim=-1, keepdim=True)
    p = torch.where(live, e / torch.where(live, l, torch.ones_like(l)), torch.zeros_like(e))
    ob = torch.matmul(p, kb[..., :dv])                                           # [Hkv, group x Sq, dv]
    o[start:start + sq, 0] = ob.reshape(hq, sq, dv).transpose(0, 1)
    row_lse = torch.where(live, m + torch.log(torch.where(live, l, torch.ones_like(l))), torch.full_like(m, float("-inf")))
    lse[start:start + sq, :, 0] = row_lse.reshape(hq, sq).t()
    pmax[start:start + sq, :, 0] = p.amax(dim=-1).reshape(hq, sq).t()
    p2sum[start:start + sq, :, 0] = p.pow(2).sum(dim=-1).reshape(hq, sq).t()
    start += sq
  return (o, lse, pmax, p2sum), ((amax, (sumsq / cnt) ** 0.5) if cnt else (1.0, 1.0))


def reference(c: dict, t: dict):
  """-> ``(check's tuple, one row per query token; the visible-value statistics; the expected storage after the append)``."""
  us, storage = units(c, t)
  ref, vstat = attend_units(us, c["scale"])
  return ref, vstat, storage


def flat(c: dict, out, lse):
  """A call's ``(out, lse)`` in the reference's layout: ``out [T, 1, Hq, dv]``, ``lse [T, Hq, 1]`` — from ``[B, Sq, Hq, dv]`` / ``[B, Hq, Sq]`` of the uniform calls,
  ``[T, Hq, dv]`` / ``[Hq, T]`` of the ragged and the sparse ones."""
  if c["ragged"] or c["sparse"]:
    return out[:, None], lse.t()[:, :, None]
  return out.flatten(0, 1)[:, None], lse.permute(0, 2, 1).flatten(0, 1)[:, :, None]


def assert_model_property(c: dict, us, ref) -> None:
  """A model-like case shows what its family's docstring promises (tests/kvcache_mla_cases.py ``assert_family_property``) — on the rows the call computes on (the
  dequantised ones) and on the family reference ``ref``."""
  family, knobs, _ = mv.VARIANTS[c["model"]]
  B, (hq, hkv) = MC.MODEL_BATCH, c["heads"]
  per = len(us) // B  # units per sequence: 1, or the tokens of a sparse case
  q = torch.stack([torch.cat([us[b * per + i][0] for i in range(per)]) for b in range(B)]).permute(0, 2, 1, 3).cpu()  # [B, Hq, Sq, D]
  k = torch.stack([us[b * per][1] for b in range(B)]).permute(0, 2, 1, 3).cpu()                                         # [B, Hkv, L, D]
  sq, L = q.size(2), k.size(2)
  causal = c["causal"] or (c["tree"] and c["mask_kind"] == "tril")
  case = {"variant": c["model"], "family": family, "knobs": dict(knobs), "shape": (B, hq, hkv, sq, L, D), "causal": causal, "sq": sq, "L": L}
  rows = lambda x: x.reshape(B, sq, hq).permute(0, 2, 1).cpu()  # [T, Hq, 1] -> [B, Hq, Sq]
  MC.assert_family_property(case, q, k, (ref[0], rows(ref[1]), rows(ref[2]), rows(ref[3])))
