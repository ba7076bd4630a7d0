"""ONE float64 restatement of the KV-cache calls over 16-bit K / V caches (ffpa_attn_amd/kvcache.py: ``ffpa_attn_with_kvcache``, ``_window``, ``_softcap`` with and
without a window, ``_tree``, ``_cascade`` and ``ffpa_attn_varlen_with_kvcache`` in its four launch forms), written from their docstrings and from nothing in the
kernels, and the seeded case generator of the family sweep — ``draw_case`` / ``materialize`` / ``reference`` in the vocabulary of tests/kvcache_ref.py and
tests/kvcache_mla_family_ref.py.  Every call is the same steps: each sequence has a logical list of key / value rows — taken after the append (and its rotary)
where there is one —, a boolean visibility ``[query token, key]`` made from the case's Python values alone (bottom-right causal, the window ``(left, right)``, the
tree mask over the last keys, or everything), the cap ``c tanh(s / c)`` on the scaled scores BEFORE the mask where ``softcap > 0``
(``kvcache_softcap_ref.cap_scores``), and a float64 softmax in the operations and order of ``kvcache_ref.attend``.  The append is ``kvcache_ref.append`` /
``kvcache_varlen_ref.append``, the rotation ``kvcache_ref.rotate``, the tree visibility ``tree_ref.visible``: used, not forked.  ``reference`` returns the tuple
``kvcache_ref.check`` takes — one row per query token —, the visible-value statistics its allowance wants and the caches' expected storage after the append.
Plain torch + numpy (any device): tested without a GPU (tests/test_kvcache_family.py) and used by tests/test_kvcache_family_gpu.py.

MODEL VALUES.  One case in four takes a tests/model_values.py family laid out as cache rows (``MODEL_VARIANTS``); the property the family's docstring promises
is asserted on the float64 scores of the rows the call computes (``assert_model_property``).  Where a feature destroys a property by design the family is paired
only with calls that keep it, or the property is read where it still holds:

* a WINDOW may leave key 0 outside a row's window, and it hides nothing that weighs anything from a row whose maximum climbs towards its own position: ``sink``
  and the rising staircases are not paired with the window calls (``MODEL_WINDOW``: the falling staircases, whose largest scores sit in the FIRST tiles — the
  ones the window hides —, and ``peaked``); the properties are per row over the keys the row sees (a staircase's step is read between neighbouring tiles that
  both hold a key the row sees);
* a CAP flattens large scores: the capped calls take ``large_logits``, ``peaked`` and ``outliers`` only (``MODEL_CAP``), q is NOT scaled by ``FACTOR`` on top,
  and the property is asserted on the scores that ENTER the cap (what the kernel's tanh is fed: |s| up to 140 against c = 30 / 50);
* a TREE MASK decides over the last Sq keys only, a handful of 389: it moves the output only where those keys carry the weight — the tree call takes the RISING
  staircases, whose five largest scores are the last five keys, under a ``random`` / ``sparse`` mask (a tree word hiding the largest score);
* a ROTATION mixes the channels the families put their structure in: a model-like case appends without rotary;
* the CASCADE's sequences share their first keys: every sequence holds sequence 0's rows (q differs), and the shared prefix is a whole number of 64-key tiles,
  so that the suffix pass walks the tiles the staircase was laid out for.

No row is dropped from the comparison with float64 for any of this.  ``model_values.absorbed_margin`` belongs to rows masked wholly by a large finite BIAS
value; the KV-cache calls take no bias, so it never applies here."""

from __future__ import annotations

import random

import torch

import kvcache_ref as R
import kvcache_softcap_ref as S
import kvcache_varlen_ref as V
import model_values as mv
import tree_ref

CALLS = ("plain", "window", "softcap", "softcap_window", "tree", "cascade", "varlen_paged", "varlen_window", "varlen_softcap", "varlen_packed")
PUBLIC = {"plain": "ffpa_attn_with_kvcache", "window": "ffpa_attn_with_kvcache_window", "softcap": "ffpa_attn_with_kvcache_softcap",
          "softcap_window": "ffpa_attn_with_kvcache_softcap", "tree": "ffpa_attn_with_kvcache_tree", "cascade": "ffpa_attn_with_kvcache_cascade",
          "varlen_paged": "ffpa_attn_varlen_with_kvcache", "varlen_window": "ffpa_attn_varlen_with_kvcache", "varlen_softcap": "ffpa_attn_varlen_with_kvcache",
          "varlen_packed": "ffpa_attn_varlen_with_kvcache"}
SPLITS, PAGES, STREAMS, HEADS = R.SPLITS, R.PAGES, R.STREAMS, R.HEADS
APPENDS = ("none", "same", "few", "rotary")
# span 0; an eighth of the median length (70 keys at the most) and a quarter of it, causal; at least the longest sequence (the plain call); a non-causal pair with
# right > 0.  A model-like staircase under a window takes "tiles" instead: two KV tiles and five keys, so that a row steps between the tiles it sees
WINDOW_KINDS = ("span0", "short", "identity", "noncausal", "quarter")
CAPS = (30.0, 50.0)              # tests/test_kvcache_softcap_gpu.py CAPS and FACTOR (asserted equal in tests/test_kvcache_family_gpu.py)
FACTOR = {30.0: 32.0, 50.0: 64.0}
# the tree call's eight cases by k = seed // 10: (mask kind, tokens, a prefix no longer than the draft).  EVERY one must move the float64 output against plain
# causal (``features_off``) but the ``tril`` kind, which IS plain causal: the by-design identity, as the ``identity`` window kind is.  k = 3, 7 are model-like: a
# RISING staircase of 389 keys, whose five largest scores are the last five keys — draft keys, which a ``random`` / ``sparse`` tree word hides from most rows
TREE_PLAN = (("tree", 33, False), ("random", 17, True), ("sparse", 63, False), ("random", 8, False), ("ones", 64, False), ("tree", 8, True), ("tril", 2, False),
             ("sparse", 8, False))
SWEEP_SEEDS = tuple(range(80))
ALL_EMPTY_SEEDS = (70,)          # the deliberate all-empty edge case: every length 0 or negative, nothing appended — every row is O = 0, LSE = -inf
MODEL_VARIANTS = ("outliers", "sink", "peaked", "large_logits") + tuple(f"staircase_{d}_{s}" for d in ("up", "down") for s in mv.STAIR_STEPS)
MODEL_WINDOW = ("peaked",) + tuple(f"staircase_down_{s}" for s in mv.STAIR_STEPS)
MODEL_CAP = ("large_logits", "outliers", "peaked")
MODEL_HEADS = ((16, 1), (32, 8))
MODEL_LENS = (389, 513)          # 6 tiles of 64 keys + 5 / 8 tiles + 1; 12 tiles of 32 + 5 / 16 + 1
MODEL_BATCH = 3
# the two model-like cases of every call (module docstring: which family goes with which call)
MODEL_PLAN = {"plain": ("sink", "staircase_up_7.5"), "tree": ("staircase_up_8.5", "staircase_up_16.0"), "cascade": ("staircase_down_8.5", "sink"),
              "varlen_paged": ("staircase_down_16.0", "outliers"), "varlen_packed": ("peaked", "staircase_up_8.5"), "window": ("staircase_down_7.5", "staircase_down_8.5"),
              "varlen_window": ("staircase_down_16.0", "peaked"), "softcap": ("large_logits", "peaked"), "softcap_window": ("peaked", "large_logits"),
              "varlen_softcap": ("large_logits", "outliers")}
MUTATIONS = ("window_left", "window_right", "cap_after_mask", "tree_shift", "align", "drop_last_tile")


def traits(call: str) -> dict:
  return {"ragged": call.startswith("varlen_"), "tree": call == "tree", "cascade": call == "cascade", "windowed": "window" in call, "capped": "softcap" in call}


def block_keys(c: dict) -> int:
  """The launch's KV tile (csrc/ffpa_fwd_m16_kernel.h ``m16_block_keys``; the GPU sweep asserts it on every plan): 64 keys at a head-dim class <= 512, 32 above
  — but 128 where a CONTIGUOUS cache runs through the packed kernel at the classes 256 and 320 (a paged launch keeps 64 there: a 64-key page holds a tile)."""
  cls = c["head_dim_class"]
  return 32 if cls > 512 else 128 if not c["page"] and 256 <= cls <= 320 else 64


def kernel_of(c: dict) -> str:
  """What the plan's kernel name of a case's attention launches starts with."""
  kind = "_tree" if c["tree"] else "_softcap" if c["capped"] else "_window" if c["windowed"] else ""
  return f"ffpa_fwd_m16_{'paged' if c['page'] else 'varlen'}{kind}_kernel<{c['dtype']}, "


# ----------------------------------------------------------------------------- the sweep's cases
def draw_case(seed: int) -> dict:
  """The family sweep's case of a seed: plain Python values only.  The call is ``CALLS[seed % 10]``; with ``k = seed // 10`` the axes a call must meet (split
  counts, pages, append kinds, the stream hint) walk their values once per four (three) k, the others are cycled with co-prime strides (``kvcache_ref._cycle``);
  lengths, token counts and the data come from the seed's own generator."""
  rng = random.Random(seed * 7919 + 57)
  ci, k = seed % len(CALLS), seed // len(CALLS)
  call = CALLS[ci]
  c = {"seed": seed, "call": call, **traits(call)}
  c["dtype"] = ("bf16", "fp16")[(k + ci) % 2]
  cls = R.PAGED_HEAD_DIM_CLASSES[(seed * 4 + seed // 15) % 15]
  c["head_dim_class"] = cls
  c["D"] = D = cls if rng.random() < 0.6 else rng.randrange(cls - 56 if cls > 128 else 8, cls, 8)
  c["heads"] = HEADS[R._cycle(seed, 5, 3)]
  c["num_splits"] = SPLITS[(k + ci) % 4]
  c["stream"] = STREAMS[(k + ci // 3) % 3]
  c["page"] = page = 0 if call == "varlen_packed" else PAGES[:3][(k + ci) % 3] if call == "varlen_paged" else PAGES[(k + 2 * ci + ci // 4) % 4]
  c["layout"] = R.POOL_LAYOUTS[R._cycle(seed, 7, 5, 1)]
  c["table_layout"] = R.TABLE_LAYOUTS[R._cycle(seed, 3, 2, 1)] if page else "plain"
  c["lens_strided"] = bool(R._cycle(seed, 2, 1, 1))
  c["causal"] = False if c["tree"] else bool(R._cycle(seed // 2, 2))
  c["model"] = None
  if (k + ci // 2) % 4 == 1:  # one case in four: two k per call, four apart, so that the model-like cases meet every split count between them
    c["model"] = MODEL_PLAN[call][k // 4]
    c["heads"] = MODEL_HEADS[(k // 4 + ci) % 2]
  model = c["model"]
  c["long"] = not model and not c["tree"] and (k + ci) % 10 in (3, 6, 8)  # about one case in five (the tree call's own sweep has its long cases: tests/tree_ref.py)
  unit = page or 64
  # tokens per sequence
  chunk = not c["tree"] and not model and not c["long"] and (k + ci) % 5 == 2
  if c["ragged"] and not model:
    B = 6 + R._cycle(seed, 3)
    big = 0 if c["long"] else rng.randrange(65, 301)
    qlens = [big, 1, 0, rng.randrange(2, 6)] + [rng.choice((1, 1, 0, rng.randrange(2, 6))) for _ in range(B - 4)]
    rng.shuffle(qlens)
  else:
    B = MODEL_BATCH if model else max(1 + R._cycle(seed, 5, 2, 1), 2 if c["cascade"] else 1)
    sq = rng.randrange(65, 301) if chunk else 1 + R._cycle(seed, 6, 5, 3)
    if c["tree"]:
      sq = TREE_PLAN[k][1]
    if model and not c["tree"]:
      sq = min(sq, 5)
    qlens = [sq] * B
    if model and c["ragged"]:
      qlens = [3, 1, 5]
  c["B"], c["qlens"], c["Sq"] = B, qlens, max(qlens)
  sqmax = c["Sq"]
  # the append
  mode = "none" if seed in ALL_EMPTY_SEEDS else APPENDS[(k + ci // 2 + ci % 3 - 1) % 4]  # (a model-like case, k + ci // 2 = 1 mod 4, appends none / same / few)
  if mode == "rotary" and (c["tree"] or model):
    mode = "same"  # (the tree call has no rotary; a rotation mixes the channels a model family puts its structure in)
  if mode == "none":
    snew = [None] * B
  elif c["ragged"] or mode != "few":
    snew = list(qlens)
  else:
    snew = [(1, 3)[(k // 4) % 2]] * B
  c["append"], c["snew"] = mode, snew
  new = [n or 0 for n in snew]
  rds = [r for r in (16, D // 2 // 16 * 16, D // 16 * 16) if 0 < r <= D]
  c["rotary_dim"] = rng.choice(rds) if mode == "rotary" and rds else 0  # (0: a head dim too small to rotate: the case appends without rotary)
  c["interleaved"] = bool((k // 2 + ci) % 2)
  c["fused_qkv"] = not c["ragged"] and mode in ("same", "rotary") and bool(R._cycle(seed // 2, 2))
  # the capacity
  L = MODEL_LENS[0 if c["tree"] else (k // 4 + ci // 2) % 2] if model else 0  # (the tree call: 389 — the last tile's five keys, the staircase's top, are draft keys)
  reach = L + 10 if model else rng.randrange(2500, 6000) if c["long"] else rng.randrange(100, 1400)
  reach = max(reach, sqmax + 64)
  if c["cascade"]:
    reach = max(reach, 2 * (sqmax + max(new)) + 2 * unit + 128)
  c["pages_per_seq"] = pps = -(-reach // unit) + 1
  c["capacity"] = cap = pps * unit if page else reach + rng.randrange(0, 64)
  c["seqlen_ro"] = cap if rng.random() < 0.5 else cap + rng.randrange(1, 100)
  # the lengths before the append
  c["shared_prefix_len"] = P = 0
  edges = (0, -3, 1, unit - 1, unit, unit + 1, cap, cap + 5, cap - 1)
  if model:
    lens = [L - n for n in new]
    if c["cascade"]:
      c["shared_prefix_len"] = P = page or 128  # (whole 64-key tiles: the suffix pass walks the tiles the staircase was laid out for)
  elif c["cascade"]:
    P = unit * rng.randrange(1, max(2, (cap // 2) // unit)) if page else rng.randrange(1, cap // 2)
    c["shared_prefix_len"] = P
    room = cap - P - sqmax - max(new)
    lens = [P + sqmax + rng.randrange(0, max(1, room)) for _ in range(B)]
  elif seed in ALL_EMPTY_SEEDS:
    lens = [(0, -3)[b % 2] for b in range(B)]
  else:
    lens = []
    b_long = next(b for b in range(B) if qlens[b] >= 1)  # (the long sequence of a long case has a token that reads it)
    for b in range(B):
      few = qlens[b] <= 8
      n = rng.choice(edges) if few and rng.random() < 0.3 else rng.randrange(1, cap)
      if c["tree"] and TREE_PLAN[k][2]:
        n = rng.randrange(0, sqmax + 2)  # a SHORT prefix: the draft keys are most of what a token sees, so the mask moves the output
      if c["long"]:
        n = rng.randrange(2500, cap) if b == b_long else n
      elif not few:
        n = max(qlens[b], min(n, 1400))  # (a chunk reads a short sequence, and every token of it sees a key under causal)
      lens.append(n)
    if all(n <= 0 for n in lens):
      lens[rng.randrange(B)] = rng.randrange(1, cap)
  c["lens"] = lens
  c["bad_unused_ids"] = bool(page) and rng.random() < 0.5
  # the window, relative to the lengths drawn: it hides keys in most rows (but for the identity kind)
  c["window"], c["window_kind"] = (-1, -1), None
  if c["windowed"]:
    eff = sorted(n for n in effective_lens(c) if n > 1) or [2]
    mid, longest = eff[len(eff) // 2], eff[-1]
    kind = c["window_kind"] = WINDOW_KINDS[(k + ci // 2) % 5]
    if model and "staircase" in model:
      kind = c["window_kind"] = "tiles"  # two tiles and five keys: a row sees three tiles of the staircase, and steps between them
    if kind == "identity":
      c["window"] = (longest + rng.randrange(0, 3), -1)  # at least as long as the longest sequence: the plain call under the same ``causal``
    elif kind == "noncausal":
      c["window"], c["causal"] = (max(1, mid // 8), rng.randrange(1, 4)), False
    else:
      c["window"] = ({"span0": 0, "short": max(1, min(mid // 8, 70)), "quarter": max(1, mid // 4), "tiles": 2 * block_keys(c) + 5}[kind], 0 if k % 2 else -1)
      c["causal"] = c["causal"] or c["window"][1] < 0  # (right = -1 with causal is right = 0; without it the right side would be open: the kinds above are causal)
  c["softcap"] = CAPS[(k // 2 + ci) % 2] if c["capped"] else 0.0
  if c["tree"]:
    c["mask_kind"] = TREE_PLAN[k][0]
    c["per_sequence"] = k % 4 >= 2 and not model
    c["tree_matters"] = c["mask_kind"] != "tril"  # (tril IS the plain causal call: the by-design identity)
  return c


def effective_lens(c: dict) -> list:
  """The keys every sequence attends over: clamp(len, 0, capacity), after the append where there is one."""
  cap = c["capacity"]
  return [min(max(n, 0) + (s or 0), cap) for n, s in zip(c["lens"], c["snew"])]


def case_mask(c: dict) -> torch.Tensor:
  """The tree mask of a drawn case (CPU): ``[Sq, Sq]`` or, per sequence, ``[B, Sq, Sq]``."""
  rng = random.Random(c["seed"] * 977 + 5)
  if c["per_sequence"]:
    return torch.stack([tree_ref.draw_mask(c["mask_kind"], c["Sq"], rng) for _ in range(c["B"])])
  return tree_ref.draw_mask(c["mask_kind"], c["Sq"], rng)


def visibility(c: dict, b: int, device="cpu", mask=None, mut: "str | None" = None) -> torch.Tensor:
  """``[tokens of b, keys of b]`` bool from the case's Python values alone: token i of sequence b sits at ``pos_i = i + n - Sq_b`` (bottom-right) and sees key j
  iff ``left < 0 or j >= pos_i - left`` and ``right < 0 or j <= pos_i + right`` (``causal``: right = 0); under a tree mask every key in front of the last Sq_b
  and, of those, what the mask says.  ``mut``: one of ``MUTATIONS`` — the ways such a rule goes subtly wrong (tests/test_kvcache_family.py)."""
  n, sq = effective_lens(c)[b], c["qlens"][b]
  if c["tree"]:
    m = case_mask(c) if mask is None else mask
    m = m if m.dim() == 2 else m[b]
    if mut == "tree_shift":  # bit j read as bit j + 1
      m = torch.cat((m[:, 1:], torch.zeros_like(m[:, :1])), dim=1)
    vis = tree_ref.visible(m, 0, n, sq, device) if sq else torch.ones((0, n), dtype=torch.bool, device=device)
  else:
    left, right = c["window"]
    right = 0 if c["causal"] else right
    left, right = left + int(mut == "window_left" and left >= 0), right + int(mut == "window_right" and right >= 0)
    pos = torch.arange(sq, device=device)[:, None] + (n - sq) - int(mut == "align")
    j = torch.arange(n, device=device)[None, :]
    vis = torch.ones((sq, n), dtype=torch.bool, device=device)
    if left >= 0:
      vis = vis & (j >= pos - left)
    if right >= 0:
      vis = vis & (j <= pos + right)
  if mut == "drop_last_tile" and n:
    vis = vis.clone()
    vis[:, (n - 1) // block_keys(c) * block_keys(c):] = False
  return vis


def visible_rows(c: dict) -> tuple:
  """``(query rows that see at least one key, query rows)`` per query head of a case."""
  mask = case_mask(c) if c["tree"] else None
  return sum(int(visibility(c, b, mask=mask).any(dim=1).sum()) for b in range(c["B"])), sum(c["qlens"])


# ----------------------------------------------------------------------------- the tensors
def _model_data(c: dict):
  """``(q [B, Hq, Sq, D], k, v [B, Hkv, L, D])`` (CPU) of the case's model_values family; the staircases step at the launch's ``block_keys``."""
  family, knobs, _ = mv.VARIANTS[c["model"]]
  knobs = dict(knobs)
  if family.startswith("staircase"):
    knobs["block_keys"] = block_keys(c)
  hq, hkv = c["heads"]
  L = max(effective_lens(c))
  q, k, v = mv.FAMILIES[family]((c["B"], hq, hkv, c["Sq"], L, c["D"]), R.TORCH_DTYPE[c["dtype"]], 3000 + c["seed"], **knobs)
  if c["cascade"]:
    k, v = k[:1].expand_as(k).contiguous(), v[:1].expand_as(v).contiguous()
  return q, k, v


def materialize(c: dict, device="cpu") -> dict:
  """The tensors of a drawn case on ``device``, in its layouts: ``q`` (``[B, Sq, Hq, D]``, ragged ``[T, Hq, D]``), ``k_cache`` / ``v_cache`` (views of
  ``k_storage`` / ``v_storage``), the new ``k`` / ``v``, ``cos`` / ``sin``, ``lens``, ``table``, ``cu`` (ragged), ``tree_mask``.  EVERY row of a cache that no sequence
  holds before the append — unused pages, rows behind a length — and everything of a storage outside its views is NaN."""
  dev = torch.device(device)
  g = torch.Generator().manual_seed(c["seed"] + 1000)
  gd = torch.Generator(device=dev).manual_seed(c["seed"] + 1000)
  dtype = R.TORCH_DTYPE[c["dtype"]]
  rnd = lambda *shape: torch.randn(shape, generator=gd, device=dev, dtype=torch.float32 if dev.type == "cpu" else dtype).to(dtype)
  D, (hq, hkv), B, page, cap, qlens = c["D"], c["heads"], c["B"], c["page"], c["capacity"], c["qlens"]
  T, P = sum(qlens), c["shared_prefix_len"]
  held = [min(max(n, 0), cap) for n in c["lens"]]
  new = [s or 0 for s in c["snew"]]
  # the logical rows of every sequence: what its cache holds, then what the call appends
  if c["model"]:
    qm, km, vm = _model_data(c)
    qs = [qm[b, :, c["Sq"] - qlens[b]:].transpose(0, 1).to(dev) for b in range(B)]  # (a shorter sequence takes the LAST tokens: the alignment is bottom-right)
    rows = [(km[b].transpose(0, 1)[:held[b] + new[b]].to(dev), vm[b].transpose(0, 1)[:held[b] + new[b]].to(dev)) for b in range(B)]
  else:
    qs = [rnd(n, hq, D) for n in qlens]
    rows = [(rnd(held[b] + new[b], hkv, D), rnd(held[b] + new[b], hkv, D)) for b in range(B)]
    if P:
      rows = [(torch.cat((rows[0][0][:P], kb[P:])), torch.cat((rows[0][1][:P], vb[P:]))) for kb, vb in rows]
    if c["capped"]:
      qs = [q * FACTOR[c["softcap"]] for q in qs]  # powers of two: the 16-bit q stays exact (tests/test_kvcache_softcap_gpu.py)
  table = None
  if page:
    pps, shared = c["pages_per_seq"], P // page
    n_pages = B * (pps - shared) + shared + 3
    ids = torch.randperm(n_pages, generator=g).tolist()
    table = torch.tensor([ids[:shared] + ids[shared + b * (pps - shared):shared + (b + 1) * (pps - shared)] for b in range(B)], dtype=torch.int32)
    kc, vc = (torch.full((n_pages, page, hkv, D), float("nan"), dtype=dtype, device=dev) for _ in range(2))
  else:
    kc, vc = (torch.full((B, cap, hkv, D), float("nan"), dtype=dtype, device=dev) for _ in range(2))
  for b in range(B):
    if held[b]:
      j = torch.arange(held[b])
      at = (table[b].long()[j // page].to(dev), (j % page).to(dev)) if page else (torch.full((held[b],), b, device=dev), j.to(dev))
      kc[at], vc[at] = rows[b][0][:held[b]], rows[b][1][:held[b]]
  if page and c["bad_unused_ids"]:
    eff = effective_lens(c)
    for b in range(B):
      for j in range(max(-(-max(eff[b], held[b]) // page), P // page), c["pages_per_seq"]):
        table[b, j] = (-1, n_pages, 2 ** 31 - 1, -(2 ** 31))[(b + j) % 4]
  t = {"k": None, "v": None, "cos": None, "sin": None, "cu": None, "tree_mask": None}
  if c["append"] != "none":
    # (every sequence hands over its ``snew`` rows, the ones the capacity cuts off too: those must be dropped)
    nk, nv = [rows[b][0][held[b]:] for b in range(B)], [rows[b][1][held[b]:] for b in range(B)]
    t["k"], t["v"] = (torch.cat(nk), torch.cat(nv)) if c["ragged"] else (torch.stack(nk), torch.stack(nv))
  q = torch.cat(qs) if c["ragged"] else torch.stack(qs)
  if c["rotary_dim"]:
    ang = torch.rand((c["seqlen_ro"], c["rotary_dim"] // 2), generator=g, dtype=torch.float64) * 6.283185307179586
    t["cos"], t["sin"] = torch.cos(ang).to(dtype).to(dev), torch.sin(ang).to(dtype).to(dev)
  kview, vview, ks, vs = R.lay_out_cache(kc, vc, c["layout"])
  if not c["ragged"]:
    q, t["k"], t["v"] = R.lay_out_qkv(q, t["k"], t["v"], c["fused_qkv"])
  if c["ragged"]:
    cu = [0]
    for n in qlens:
      cu.append(cu[-1] + n)
    t["cu"] = torch.tensor(cu, dtype=torch.int32, device=dev)
  if c["tree"]:
    t["tree_mask"] = case_mask(c).to(dev)
  t.update(q=q, k_cache=kview, v_cache=vview, k_storage=ks, v_storage=vs, lens=R.lay_out_lens(torch.tensor(c["lens"], dtype=torch.int32, device=dev), c["lens_strided"]),
           table=None if table is None else R.lay_out_table(table.to(dev), c["table_layout"]))
  return t


# ----------------------------------------------------------------------------- the calls, restated
def units(c: dict, t: dict, mut: "str | None" = None):
  """-> ``(units, caches)``: per sequence ``(q [tokens, Hq, D] — the rotated copy, rounded once to q's dtype —, K rows [n, Hkv, D], V rows, visibility
  [tokens, n])`` on the caches AFTER the append, and ``caches = (k_view, v_view, k_storage, v_storage, rotated rows)``: clones of the case's storages with the new
  rows written where the docstrings say (``kvcache_ref.append`` / ``kvcache_varlen_ref.append``)."""
  ks = t["k_storage"].clone()
  vs = ks if t["v_storage"] is t["k_storage"] else t["v_storage"].clone()
  kview, vview = R.reviewed(t["k_cache"], t["k_storage"], ks), R.reviewed(t["v_cache"], t["v_storage"], vs)
  q, rotated, dev = t["q"], [], t["q"].device
  if t["k"] is not None:
    if c["ragged"]:
      q_rot, lens, rotated = V.append(kview, vview, t["k"], t["v"], t["cu"].tolist(), c["lens"], t["table"], t["cos"], t["sin"], c["interleaved"], c["causal"], q=q)
    else:
      q_rot, lens, rotated = R.append(kview, vview, t["k"], t["v"], c["lens"], t["table"], t["cos"], t["sin"], c["interleaved"], c["causal"], q=q)
    assert lens == effective_lens(c), (lens, effective_lens(c))
    if q_rot is not None:
      q = q_rot.to(t["q"].dtype)
  out, start = [], 0
  for b, (n_tok, n) in enumerate(zip(c["qlens"], effective_lens(c))):
    qb = q[start:start + n_tok] if c["ragged"] else q[b]
    start += n_tok
    kb, vb = R.gather(kview, vview, t["table"], b, n)
    out.append((qb, kb.double(), vb.double(), visibility(c, b, dev, t["tree_mask"], mut)))
  return out, (kview, vview, ks, vs, rotated)


def unit_scores(c: dict, u, capped: bool = True) -> torch.Tensor:
  """The float64 scores ``[Hkv, group x tokens, n]`` of a unit (rows (head in group, token)), scaled, capped where the case caps and ``capped``; NOT masked."""
  q, kb, _, _ = u
  sq, hq, d = q.shape
  hkv = kb.size(1)
  qb = q.double().transpose(0, 1).reshape(hkv, (hq // hkv) * sq, d)
  s = torch.matmul(qb, kb.transpose(0, 1).transpose(1, 2)) * d ** -0.5
  return S.cap_scores(s, c["softcap"]) if capped else s


def attend_units(c: dict, us, mut: "str | None" = None):
  """``kvcache_ref.attend``'s float64 softmax — the same operations in the same order — over the units of a case -> ``(check's tuple with one row per query token:
  o [T, 1, Hq, D], lse [T, Hq, 1], pmax, p2sum; (largest |v|, RMS of v) over the rows the units hold)``.  A hidden key's V may be anything (its weight is an
  exact 0)."""
  T = sum(u[0].size(0) for u in us)
  hq, d, dev = us[0][0].size(1), us[0][0].size(2), us[0][0].device
  o = torch.zeros((T, 1, hq, d), dtype=torch.float64, device=dev)
  lse = torch.full((T, hq, 1), float("-inf"), dtype=torch.float64, device=dev)
  pmax = torch.zeros((T, hq, 1), dtype=torch.float64, device=dev)
  p2sum = torch.zeros((T, hq, 1), dtype=torch.float64, device=dev)
  amax, sumsq, cnt, start = 0.0, 0.0, 0, 0
  for u in us:
    q, kb, vb, vis = u
    sq, n = q.size(0), kb.size(0)
    if n:
      amax, sumsq, cnt = max(amax, float(vb.abs().max())), sumsq + float(vb.pow(2).sum()), cnt + vb.numel()
    if n == 0 or sq == 0:
      start += sq
      continue
    group = hq // kb.size(1)
    seen = vis.repeat(group, 1)[None]
    if mut == "cap_after_mask":
      s = S.cap_scores(unit_scores(c, u, capped=False).masked_fill(~seen, float("-inf")), c["softcap"])
    else:
      s = unit_scores(c, u).masked_fill(~seen, float("-inf"))
    m = s.amax(dim=-1, keepdim=True)
    live = torch.isfinite(m)
    e = torch.exp(s - torch.where(live, m, torch.zeros_like(m)))
    l = e.sum(dim=-1, keepdim=True)
    p = torch.where(live, e / torch.where(live, l, torch.ones_like(l)), torch.zeros_like(e))
    ob = torch.matmul(p, vb.transpose(0, 1))                                     # [Hkv, group x Sq, D]
    o[start:start + sq, 0] = ob.reshape(hq, sq, d).transpose(0, 1)
    row_lse = torch.where(live, m + torch.log(torch.where(live, l, torch.ones_like(l))), torch.full_like(m, float("-inf")))
    lse[start:start + sq, :, 0] = row_lse.reshape(hq, sq).t()
    pmax[start:start + sq, :, 0] = p.amax(dim=-1).reshape(hq, sq).t()
    p2sum[start:start + sq, :, 0] = p.pow(2).sum(dim=-1).reshape(hq, sq).t()
    start += sq
  return (o, lse, pmax, p2sum), ((amax, (sumsq / cnt) ** 0.5) if cnt else (1.0, 1.0))


def reference(c: dict, t: dict, mut: "str | None" = None):
  """-> ``(check's tuple, one row per query token; the visible-value statistics; (k_view, v_view, k_storage, v_storage, rotated rows) after the append)``."""
  us, caches = units(c, t, mut)
  ref, vstat = attend_units(c, us, mut)
  return ref, vstat, caches


def flat(c: dict, out, lse):
  """A call's ``(out, lse)`` in the reference's layout: ``out [T, 1, Hq, D]``, ``lse [T, Hq, 1]`` — from ``[B, Sq, Hq, D]`` / ``[B, Hq, Sq]`` of the uniform calls,
  ``[T, Hq, D]`` / ``[Hq, T]`` of the ragged ones."""
  if c["ragged"]:
    return out[:, None], lse.t()[:, :, None]
  return out.flatten(0, 1)[:, None], lse.permute(0, 2, 1).flatten(0, 1)[:, :, None]


def moved_share(c: dict, ref, other, vstat) -> float:
  """The share of the non-empty rows of ``ref`` in which ``other`` (the same case with a feature off) differs by more than 10 allowances
  (tests/test_kvcache_softcap_gpu.py ``_cap_matters``: at least 0.5 says the feature matters)."""
  import numpy as np

  o_ref, lse_ref, pmax, p2sum = (x.cpu().numpy() for x in ref)
  stat = lambda x: np.transpose(x, (0, 2, 1))
  half_ulp, flip = R.allowance(o_ref, stat(pmax), stat(p2sum), vstat, c["dtype"], noise=True)
  rows = (np.abs(other[0].cpu().numpy() - o_ref) > 10.0 * (half_ulp + flip)).any(axis=-1)
  live = np.isfinite(stat(lse_ref))
  return float(rows[live].mean()) if live.any() else 0.0


def features_off(c: dict) -> list:
  """The case with each feature its call is named for switched off, one at a time — the cap 0, the window open, the tree mask plain causal — as ``(name, case)``.
  Left out where the feature is an identity by design: the ``identity`` window kind; a cap under span 0 (a row sees ONE key: no cap moves a softmax over one
  key); the ``tril`` mask kind, which is plain causal itself (``tree_matters`` is False for it alone)."""
  if c["tree"]:
    return [("tree mask", dict(c, mask_kind="tril", per_sequence=False))] if c["tree_matters"] else []
  out = []
  if c["capped"] and c["window_kind"] != "span0":
    out.append(("cap", dict(c, softcap=0.0)))
  if c["windowed"] and c["window_kind"] != "identity":
    out.append(("window", dict(c, window=(-1, -1))))
  return out


# ----------------------------------------------------------------------------- model values: what a family promises, on the rows the call computes
def assert_model_property(c: dict, us) -> dict:
  """The property the family's docstring promises (the thresholds of tests/test_model_values_ref.py) on the float64 scores of the case's units, over the keys each
  row SEES — for a capped call on the scores that enter the cap (module docstring).  -> the figures it read (printed by the tests)."""
  family, knobs, _ = mv.VARIANTS[c["model"]]
  name = f"seed {c['seed']} {c['call']} {c['model']}"
  pm, p0, tops, diffs, vmax, vch = [], [], [], [], 0.0, 0.0
  bc = block_keys(c)
  for u in us:
    q, kb, vb, vis = u
    if q.size(0) == 0:
      continue
    group = q.size(1) // kb.size(1)
    seen = vis.repeat(group, 1)[None]
    s = unit_scores(c, u, capped=False).masked_fill(~seen, float("-inf"))
    live = seen.any(dim=-1).expand(s.shape[:2])
    p = torch.softmax(s[live], dim=-1)
    pm.append(p.amax(dim=-1))
    sees0 = seen[..., 0].expand(s.shape[:2])[live]
    p0.append(p[sees0][:, 0])
    tops.append(float(s[torch.isfinite(s)].abs().max()))
    vmax, vch = max(vmax, float(vb.abs().max())), max(vch, float(vb[..., mv.V_OUTLIER_CHANNEL].abs().max()))
    if family.startswith("staircase"):
      s2 = s[live] * mv.LOG2E
      n = s2.size(-1)
      tmax = torch.stack([s2[:, i * bc:(i + 1) * bc].amax(dim=-1) for i in range(-(-n // bc))], dim=-1)
      both = torch.isfinite(tmax[:, 1:]) & torch.isfinite(tmax[:, :-1])
      diffs.append(((tmax[:, 1:] - tmax[:, :-1]) * (1 if family == "staircase_up" else -1))[both])
  pm, p0 = torch.cat(pm), torch.cat(p0)
  fig = {"rows": int(pm.numel()), "mean pmax": float(pm.mean()), "top |s|": max(tops)}
  if family in ("outliers", "sink"):
    assert fig["mean pmax"] >= 0.4, (name, fig)
    assert vmax >= 100.0 and vch == vmax, (name, vmax, vch)
  if family == "sink":
    fig.update({"p0 >= 0.5": float((p0 >= 0.5).double().mean()), "p0 <= 1e-6": float((p0 <= 1e-6).double().mean())})
    assert p0.numel() == pm.numel() and fig["p0 >= 0.5"] >= 0.04 and fig["p0 <= 1e-6"] >= 0.25, (name, fig)
  if family == "peaked":
    assert fig["mean pmax"] >= 0.5, (name, fig)
  if family == "large_logits":
    assert 55.0 <= fig["top |s|"] <= 140.0, (name, fig)
  if family.startswith("staircase"):
    d = torch.cat(diffs)
    step = knobs["step"]
    fig.update({"tile steps": int(d.numel()), "worst |step - want|": float((d - step).abs().max())})
    # the staircase crosses the launch's tile boundaries: every row that sees two neighbouring tiles steps between them, on its side of the threshold
    assert d.numel() >= pm.numel() and fig["worst |step - want|"] <= 0.25, (name, fig)
    assert bool(((d > mv.RESCALE_THRESHOLD) == (step > mv.RESCALE_THRESHOLD)).all()), name
  return fig
