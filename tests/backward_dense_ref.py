"""ONE float64 restatement of the dense call a training step differentiates (``ffpa_attn_func`` with a gradient: batches, GQA, every mask form the public call
takes, ``is_causal``, dropout) and the seeded case generator of its sweep — ``draw_case`` / ``materialize`` / ``reference`` in the vocabulary of
tests/kvcache_family_ref.py.  Written from the call's docstring and from nothing in ``backward.py``: ``S = scale Q K^T`` with GQA by ``repeat_interleave``; the mask
added EXACTLY as it was passed (bool: 0 / -inf; additive: its value in the math dtype — an fp32 bias next to 16-bit queries is never rounded to the queries'
dtype); the tail-aligned causal mask; ``P = softmax(S)``; ``O = (P o keep / (1 - p)) V`` (the LSE is the undropped one); gradients by autograd for q, k, v and
the bias where it asks for one.  ``keep`` is ``ffpa_attn_amd.philox.dropout_keep_mask`` at the element index ``((b Hq + h) Nq + r) Nkv + j`` (built here) with the
seed and offset the call reserved; tests/test_backward_dense_family.py ties that function to the C oracle's Philox and tests/test_backward_dense_family_gpu.py to
the kernel's own mask, whole tensors, so that the reference may use it.  Plain torch (any device): tested without a GPU on small copies of the cases (``shrink``).

THE BASELINE (``reference(..., math=torch.float32, out_dtype=<the queries' dtype>)``) is the same math in float32 on the storage-dtype inputs — the fp32 bias
stays fp32 —, the same ``keep``, O and every gradient rounded to the queries' 16-bit dtype: what SDPA's math backend computes, and the baseline
tests/test_backward_f64_gpu.py uses for losses of the LSE.  (SDPA itself takes no fp32 mask next to 16-bit queries and cannot be handed a keep mask.)  The
baseline's dbias is rounded to the QUERIES' dtype too, also where the bias is fp32: SDPA returns a bias gradient in the only bias dtype it takes, and a float32
dbias would be a baseline without the storage rounding every other gradient of it carries.  The library's dbias is compared in the bias's own shape and dtype.

THE DRAW.  48 seeds: ``kind = KINDS[seed % 12]``, the occurrence ``o = seed // 12`` picks the dtype (``o % 2``) and the head-dim class (``o // 2``: 320 / 456 /
512, which aten's backward may serve, or 576 / 768 / 1024, the recompute's alone), so every mask kind meets both dtypes and both classes.  B 2 or 3; heads (4, 4),
(4, 2), (8, 1), (6, 3); prefill rows 512 ... 640 against 512 ... 777 keys (the smallest the kernel serves: ``FFPAAttnMeta.fallback``), most key counts no multiple
of 8; one case in four is a decode step (1 or 5 rows) against 512 ... 777 or 4096 keys (the library's own KV split and merge write the LSE).  Each additive kind
asks once for the bias gradient.  Dropout (p 0.1 / 0.5) on one case in three, by ``DROPOUT_PLAN``: twice with ``is_causal``, three times with a bool mask, five
times with an fp32 bias; the generator's offset is a nonzero multiple of four in most of them (torch's generator refuses any other offset, so the public call
never sees one: the offsets inside a Philox quad are tests/test_backward_dense_family_gpu.py's keep-mask test and the CPU tests').  aten's backward on ROCm
serves head dims up to 512 and refuses a row count that is no multiple of 8 (the call then takes the recompute): every kind has one case or two it can serve
(``aten_may_serve``: the first head-dim class, no dropout, no decode), and those draw their rows from the multiples of 8; the others draw any row count.

Rows without a visible key are NOT drawn: the dense call returns NaN for them as SDPA does, and no gradient contract is stated for them (every key-padding length
is >= 1, every bool row keeps a key)."""

from __future__ import annotations

import random

import torch

import model_values as mv
from ffpa_attn_amd.philox import dropout_keep_mask

KINDS = ("none", "causal", "bool_keypad", "bool_rows", "add16_rows", "add16_full", "add16_heads", "fp32_rows", "fp32_full", "fp32_heads", "fp32_keypad_min",
         "lowdim")
ADDITIVE = ("add16_rows", "add16_full", "add16_heads", "fp32_rows", "fp32_full", "fp32_heads")
LOWDIM = (("2d", "add16"), ("3d", "fp32"), ("2d", "bool"), ("3d", "add16"))  # the ``lowdim`` kind by occurrence: (dims of the mask as passed, its values)
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
HEADS = ((4, 4), (4, 2), (8, 1), (6, 3))
D_CLASSES = ((320, 456, 512), (576, 768, 1024))
SWEEP_SEEDS = tuple(range(48))
# the kinds that run under dropout, by occurrence: 16 of 48 cases
DROPOUT_PLAN = (("bool_rows", "add16_heads", "fp32_heads", "add16_full"), ("bool_keypad", "fp32_full", "add16_rows", "lowdim"),
                ("none", "causal", "fp32_rows", "fp32_keypad_min"), ("causal", "bool_rows", "add16_full", "fp32_heads"))
ALIBI_SEED = 9  # fp32 [1, Hq, 1, Nkv] at one query row: tests/model_values.py's ALiBi of a decode step
OFFSETS = (0, 4, 12, 4 * ((1 << 20) + 1), 4 * ((1 << 33) + 5))  # what the generator is set to before a dropout call (multiples of four: module docstring)
FP32_SCALE, ADD16_SCALE = 2.0, 1.0  # additive values ~ N(0, scale)


def mask_form(c: dict) -> tuple:
  """(values, shape as passed) of a case's mask: values ``None`` / ``bool`` / ``add16`` / ``fp32`` / ``fp32_min``."""
  B, (hq, _), nq, nkv, kind = c["B"], c["heads"], c["Nq"], c["Nkv"], c["kind"]
  if kind in ("none", "causal"):
    return None, None
  if kind == "lowdim":
    dims, values = LOWDIM[c["seed"] // 12]
    return values, (nq, nkv) if dims == "2d" else (B, nq, nkv)
  shape = {"keypad": (B, 1, 1, nkv), "rows": (1, 1, nq, nkv), "full": (B, hq, nq, nkv), "heads": (1, hq, 1, nkv), "min": (B, 1, 1, nkv)}[kind.split("_")[-1]]
  return {"bool": "bool", "add16": "add16", "fp32": "fp32_min" if kind == "fp32_keypad_min" else "fp32"}[kind.split("_")[0]], shape


def draw_case(seed: int) -> dict:
  """The sweep's case of a seed: plain Python values only (module docstring)."""
  rng = random.Random(seed * 7919 + 101)
  ki, o = seed % len(KINDS), seed // len(KINDS)
  kind = KINDS[ki]
  c = {"seed": seed, "kind": kind, "dtype": ("bf16", "fp16")[o % 2], "d_class": o // 2, "D": D_CLASSES[o // 2][(ki + o) % 3], "B": 2 + (ki + o) % 2,
       "heads": HEADS[(ki + ki // 4 + o) % 4], "causal": kind == "causal"}
  c["decode"] = decode = (ki + o) % 4 == 1
  c["dropout_p"] = (0.1, 0.5)[(ki + o) % 2] if kind in DROPOUT_PLAN[o] else 0.0
  # aten's backward on ROCm serves head dims up to 512 and row counts that are a multiple of 8 (it refuses the others, and the call falls back to the recompute):
  # a case it could serve draws such a row count, so that every mask kind meets that route with a batch
  c["aten_may_serve"] = o // 2 == 0 and not decode and c["dropout_p"] == 0.0
  if decode:
    c["Nq"] = 5 if kind == "causal" else 1 if seed == ALIBI_SEED else rng.choice((1, 5))
    c["Nkv"] = 4096 if (ki // 4 + o) % 2 == 0 else rng.randrange(513, 777)
  elif c["aten_may_serve"]:
    c["Nq"] = rng.choice((512, 640)) if rng.random() < 0.3 else rng.randrange(520, 640, 8)
    c["Nkv"] = rng.choice((512, 777)) if rng.random() < 0.3 else rng.randrange(513, 777)
  else:
    c["Nq"] = rng.choice((512, 640)) if rng.random() < 0.3 else rng.randrange(513, 640)
    c["Nkv"] = rng.choice((512, 777)) if rng.random() < 0.3 else rng.randrange(513, 777)
  if c["causal"]:
    c["Nkv"] = max(c["Nkv"], c["Nq"])
  values, _ = mask_form(c)
  c["alibi"] = seed == ALIBI_SEED
  c["bias_grad"] = (kind in ADDITIVE and o == ki % 4) or (kind == "lowdim" and o == 3)
  c["bias_scale"] = FP32_SCALE if values == "fp32" else ADD16_SCALE
  # key padding: per batch the side that is padded and the share of the keys that stay (at least one key: ``kept_keys``)
  first = rng.randrange(2)
  c["pad"] = [(("right", "left")[(first + b) % 2], rng.uniform(0.3, 0.95)) for b in range(c["B"])]
  c["pad_delta"] = 0
  c["rng_seed"] = rng.getrandbits(62) if rng.random() < 0.5 else rng.randrange(1, 1000)
  c["rng_offset"] = OFFSETS[(ki + 2 * o + 1) % len(OFFSETS)]
  return c


def shrink(c: dict, **over) -> dict:
  """A small copy of a case for the CPU tests: the same batch, heads, mask kind, dtypes, dropout and padding shares; a handful of rows and keys (Nkv > Nq, so
  ``is_causal`` stands; decode rows stay), head dim 16."""
  s = dict(c, Nq=c["Nq"] if c["Nq"] <= 7 else 17 + c["Nq"] % 16, Nkv=33 + c["Nkv"] % 24, D=16)
  s.update(over)
  return s


def features_off(c: dict, mask: bool = True, dropout: bool = True) -> dict:
  """The case without its mask (and ``is_causal``) and / or without its dropout: what a backward that dropped the feature would compute."""
  s = dict(c)
  if mask:
    s.update(kind="none", causal=False, bias_grad=False, alibi=False)
  if dropout:
    s["dropout_p"] = 0.0
  return s


def kept_keys(c: dict) -> list:
  """Per batch the (first, one past the last) key a key-padding mask keeps."""
  out = []
  for side, share in c["pad"]:
    n = min(c["Nkv"], max(1, int(share * c["Nkv"])) + c["pad_delta"])
    out.append((0, n) if side == "right" else (c["Nkv"] - n, c["Nkv"]))
  return out


def materialize(c: dict, device="cpu") -> dict:
  """The tensors of a case, drawn on the CPU from the case's seed (the same values on every device): q, k, v and dO in the storage dtype, the mask in the form
  the public call is handed (``mask``: 2-D / 3-D / 4-D, or None), the dropout triple ``(p, seed, offset)`` or None."""
  gen = torch.Generator().manual_seed(c["seed"] * 104729 + 7)
  dtype = DTYPES[c["dtype"]]
  B, (hq, hkv), nq, nkv, D = c["B"], c["heads"], c["Nq"], c["Nkv"], c["D"]
  randn = lambda *shape: torch.randn(*shape, generator=gen, dtype=torch.float32)  # noqa: E731
  t = {"q": randn(B, hq, nq, D).to(dtype), "k": randn(B, hkv, nkv, D).to(dtype), "v": randn(B, hkv, nkv, D).to(dtype), "go": randn(B, hq, nq, D).to(dtype)}
  values, shape = mask_form(c)
  mask = None
  if c["kind"] in ("bool_keypad", "fp32_keypad_min"):
    keep = torch.zeros(shape, dtype=torch.bool)
    for b, (a, e) in enumerate(kept_keys(c)):
      keep[b, 0, 0, a:e] = True
    mask = keep if values == "bool" else torch.zeros(shape, dtype=torch.float32).masked_fill_(~keep, torch.finfo(torch.float32).min)
  elif values == "bool":
    mask = torch.rand(shape, generator=gen) < 0.7
    rows = torch.arange(nq)
    mask[..., rows, (rows * 7) % nkv] = True  # (every row keeps a key)
  elif c.get("alibi"):
    mask = mv.alibi((B, hq, hkv, nq, nkv, D), dtype, c["seed"], bias_dtype=torch.float32)[3]
    assert mask.shape == shape and mask.dtype == torch.float32
  elif values is not None:
    mask = (randn(*shape) * c["bias_scale"]).to(torch.float32 if values == "fp32" else dtype)
  t["mask"] = mask
  t = {n: x.to(device) if x is not None else None for n, x in t.items()}
  t["dropout"] = (c["dropout_p"], c["rng_seed"], c["rng_offset"]) if c["dropout_p"] > 0.0 else None
  return t


def mask4(c: dict, mask):
  """The 4-D broadcasting view of a mask as passed: 2-D -> [1, 1, Nq, Nkv], 3-D -> [B, 1, Nq, Nkv] (the public call's documented reading)."""
  if mask is None or mask.dim() == 4:
    return mask
  return mask.view(1, 1, *mask.shape) if mask.dim() == 2 else mask.view(mask.size(0), 1, *mask.shape[1:])


def element_index(c: dict, device) -> torch.Tensor:
  """int64 [B, Hq, Nq, Nkv]: the logical score index ``((b Hq + h) Nq + r) Nkv + j`` the dropout convention draws at."""
  B, (hq, _), nq, nkv = c["B"], c["heads"], c["Nq"], c["Nkv"]
  ar = lambda n, *view: torch.arange(n, dtype=torch.int64, device=device).view(*view)  # noqa: E731
  return ((ar(B, B, 1, 1, 1) * hq + ar(hq, 1, hq, 1, 1)) * nq + ar(nq, 1, 1, nq, 1)) * nkv + ar(nkv, 1, 1, 1, nkv)


def keep_mask(c: dict, t: dict, device):
  """bool [B, Hq, Nq, Nkv] (or None): the elements the call's dropout keeps."""
  if t["dropout"] is None:
    return None
  p, seed, offset = t["dropout"]
  return dropout_keep_mask(seed, offset, element_index(c, device), p)


def reference(c: dict, t: dict, math=torch.float64, out_dtype=None, keep=None) -> dict:
  """O, LSE and the gradients of ``sum(O o dO)`` by autograd through explicit math in ``math`` (float64: the reference; float32 with ``out_dtype``: the
  baseline, O and the gradients rounded to ``out_dtype``).  ``grads``: dq, dk, dv and — where the case asks for it — dbias in the shape the mask was passed in."""
  q, k, v = (t[n].to(math).requires_grad_() for n in ("q", "k", "v"))
  (hq, hkv), nq, nkv = c["heads"], c["Nq"], c["Nkv"]
  g = hq // hkv
  s = (q @ k.repeat_interleave(g, 1).transpose(-1, -2)) * (c["D"] ** -0.5)
  leaves = [q, k, v]
  mask = t["mask"]
  if mask is not None and mask.dtype == torch.bool:
    s = s.masked_fill(~mask4(c, mask), float("-inf"))
  elif mask is not None:
    bias = mask.to(math)  # exactly the values passed: no rounding to the queries' dtype
    if c["bias_grad"]:
      bias = bias.clone().requires_grad_()
      leaves.append(bias)
    s = s + mask4(c, bias)
  if c["causal"]:
    cols, rows = torch.arange(nkv, device=s.device).view(1, -1), torch.arange(nq, device=s.device).view(-1, 1)
    s = s.masked_fill(cols > rows + (nkv - nq), float("-inf"))
  lse = torch.logsumexp(s, -1)
  p = torch.softmax(s, -1)
  if t["dropout"] is not None:
    keep = keep_mask(c, t, s.device) if keep is None else keep
    p = p * (keep.to(math) / (1.0 - t["dropout"][0]))
  o = p @ v.repeat_interleave(g, 1)
  if out_dtype is not None:
    o = o.to(out_dtype)
  grads = torch.autograd.grad(o, leaves, t["go"].to(o.dtype))
  if out_dtype is not None:
    grads = [x.to(out_dtype) for x in grads]
  return {"o": o.detach(), "lse": lse.detach(), "grads": tuple(grads)}


def baseline(c: dict, t: dict, keep=None) -> dict:
  return reference(c, t, math=torch.float32, out_dtype=DTYPES[c["dtype"]], keep=keep)
