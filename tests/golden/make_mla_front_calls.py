"""Record tests/golden/mla_front_calls.json: what the Python front end of the MLA latent-cache family answers, call by call, WITHOUT a device.

    PYTHONPATH=<checkout> python tests/golden/make_mla_front_calls.py [--out PATH]

The six entry points (ffpa_attn_with_kvcache_mla, _mla_fp8, _mla_tree and their ffpa_attn_varlen_* twins) are recorded three ways:

* signatures: ``str(inspect.signature(f))`` (the address in the repr of the "required" sentinel blanked: it changes from run to run) and ``f.__doc__``;
* refusals: a smallest valid argument set on CPU tensors, one named fault (or two, for the ORDER of neighbouring checks) applied to it, and the exception's type
  name and full message.  The recorder proves its own coverage: it finds every ``raise`` of the checked functions in the source with ``ast`` and asserts that a
  single-fault row ended on each of them (by the traceback's line; no line number is stored);
* served calls: the same argument sets on META tensors under a ``TorchDispatchMode`` -> the sequence of ``ffpa_attn::*`` ops with every argument (a tensor as
  ``who:dtype[shape](strides)@device``, ``who`` the caller's argument it IS — Python identity — or ``new``; anything else as ``repr:type``) and the returned
  tensors.  The file packs rows that answer alike into one entry (``pack`` / ``unpack``).

tests/test_kvcache_mla_front.py replays every row through ``replay`` and compares for equality.  The committed list was recorded from the commit BEFORE the front
end was folded into one checker and one step: signatures, docstrings, order and wording of every refusal and every op argument are pinned to that."""

import argparse
import ast
import inspect
import itertools
import json
import os
import re
import traceback

import torch
from torch.utils._python_dispatch import TorchDispatchMode

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "mla_front_calls.json")

UNIFORM = ("ffpa_attn_with_kvcache_mla", "ffpa_attn_with_kvcache_mla_fp8", "ffpa_attn_with_kvcache_mla_tree")
RAGGED = ("ffpa_attn_varlen_with_kvcache_mla", "ffpa_attn_varlen_with_kvcache_mla_fp8", "ffpa_attn_varlen_with_kvcache_mla_tree")
FUNCS = UNIFORM + RAGGED

HQ, HKV, D, DV = 16, 1, 576, 512
PAGES, PAGE, PER_SEQ, CAP = 4, 64, 2, 128  # the pool: 4 pages of 64 rows, 2 pages per sequence; the contiguous form: capacity 128
B_UNIFORM, SQ = 2, 3
RAGGED_LENS = (1, 0, 3)
SCALE, KV_SCALE = 0.125, 0.5
_DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}


def _kvcache():
  from ffpa_attn_amd import kvcache

  return kvcache


# ----------------------------------------------------------------------------------------------------------------------------- the argument sets
def base_args(func, layout="paged", dtype="bf16", device="cpu", kv="given", lens="tensor", mask="bool2", empty=None):
  """The smallest valid keyword set of ``func`` (every parameter can be passed by keyword).  ``kv``: "none" | "given" | "empty" (Snew = 0, uniform calls);
  ``lens``: cache_seqlens as a "tensor" or an "int" (uniform calls); ``mask``: "bool2" [W, W] | "bool3" [B, W + 1, W + 1] | "words" int64 [B, W] | "int32" (a bad
  one, for the empty cases that never look at it); ``empty``: None | "B0" | "Sq0" (uniform) | "T0" (ragged)."""
  ragged, fp8, tree = func in RAGGED, func.endswith("_fp8"), func.endswith("_tree")
  dt = _DTYPES[dtype]

  def z(*shape, dtype=dt):
    return torch.zeros(*shape, dtype=dtype, device=device)

  if ragged:
    seqs = (0, 0, 0) if empty == "T0" else RAGGED_LENS
    B, T = len(seqs), sum(seqs)
    a = {"q": z(T, HQ, D)}
    new_shape = (T, HKV, D)
  else:
    B, Sq = (0 if empty == "B0" else B_UNIFORM), (0 if empty == "Sq0" else SQ)
    a = {"q": z(B, Sq, HQ, D)}
    new_shape = (B, 0 if kv == "empty" else SQ, HKV, D)
  cache_dt = torch.float8_e4m3fn if fp8 else dt
  a["kv_cache"] = z(PAGES, PAGE, HKV, D, dtype=cache_dt) if layout == "paged" else z(B, CAP, HKV, D, dtype=cache_dt)
  a["head_dim_v"] = DV
  if ragged:
    a["cu_seqlens_q"] = torch.tensor([0, *itertools.accumulate(seqs)], dtype=torch.int32).to(device)
    a["max_seqlen_q"] = max(seqs)
  a["cache_seqlens"] = 5 if lens == "int" else z(B, dtype=torch.int32)
  if layout == "paged":
    a["block_table"] = z(B, PER_SEQ, dtype=torch.int32)
  if kv != "none":
    a["kv"] = z(*new_shape)
  a["softmax_scale"] = SCALE
  if fp8:
    a["kv_scale"] = KV_SCALE
  if tree:
    W = SQ
    a["tree_mask"] = {"bool2": lambda: z(W, W, dtype=torch.bool), "bool3": lambda: z(B, W + 1, W + 1, dtype=torch.bool),
                      "words": lambda: z(B, W, dtype=torch.int64), "int32": lambda: z(W, W, dtype=torch.int32)}[mask]()
  return a


# ----------------------------------------------------------------------------------------------------------------------------- the faults
def _meta(t):
  return torch.empty_like(t, device="meta")


def _grad(t):
  return t.clone().requires_grad_()


def _strided(t):  # the same shape with a last-dimension stride of 2
  return torch.zeros(*t.shape[:-1], 2 * t.size(-1), dtype=t.dtype, device=t.device)[..., ::2]


def _other16(t):
  return t.to(torch.float16 if t.dtype == torch.bfloat16 else torch.bfloat16)


def _heads(n, dim):
  def f(t):
    shape = [-1] * t.dim()
    shape[dim] = n
    return t.expand(*shape)

  return f


_POP = object()
# name -> (argument, a value that REPLACES it | a function that TRANSFORMS the tensor it holds).  Two faults on one argument combine only if both transform.
FAULTS = {
  "scale_missing": ("softmax_scale", _POP), "scale_str": ("softmax_scale", "0.125"),
  "q_list": ("q", [1.0]), "q_grad": ("q", _grad), "q_f32": ("q", lambda t: t.float()), "q_rank": ("q", lambda t: t[0]),
  "q_sq65": ("q", lambda t: torch.zeros(t.size(0), 65, *t.shape[2:], dtype=t.dtype, device=t.device)),
  "cache_none": ("kv_cache", None), "cache_grad": ("kv_cache", _grad), "cache_dim": ("kv_cache", lambda t: t[..., :512]), "cache_heads": ("kv_cache", _heads(3, 2)),
  "cache_meta": ("kv_cache", _meta), "cache_page32": ("kv_cache", lambda t: t[:, :32]), "cache_batch": ("kv_cache", lambda t: t[:1]),
  "cache_cap100": ("kv_cache", lambda t: t[:, :100]), "cache_16bit": ("kv_cache", lambda t: t.to(torch.bfloat16)),
  "kv_list": ("kv", [1.0]), "kv_grad": ("kv", _grad), "kv_dtype": ("kv", _other16), "kv_meta": ("kv", _meta), "kv_heads": ("kv", _heads(2, -2)),
  "kv_stride": ("kv", _strided),
  "hdv_float": ("head_dim_v", 512.0), "hdv_100": ("head_dim_v", 100), "hdv_256": ("head_dim_v", 256),
  "splits_neg": ("num_splits", -1),
  "bt_int64": ("block_table", lambda t: t.long()), "bt_nopages": ("block_table", lambda t: t[:, :0]), "bt_meta": ("block_table", _meta),
  "lens_neg": ("cache_seqlens", -1), "lens_str": ("cache_seqlens", "5"), "lens_list": ("cache_seqlens", [0, 0, 0]),
  "lens_int64": ("cache_seqlens", lambda t: t.long()), "lens_short": ("cache_seqlens", lambda t: t[:1]),
  "cu_list": ("cu_seqlens_q", [0, 1, 1, 4]), "cu_int64": ("cu_seqlens_q", lambda t: t.long()), "cu_rank": ("cu_seqlens_q", lambda t: t[None]),
  "max_neg": ("max_seqlen_q", -1), "max_65": ("max_seqlen_q", 65),
  "unserved": ("window_size", (1, 1)),
  "kvscale_tensor": ("kv_scale", torch.tensor(1.0)), "kvscale_str": ("kv_scale", "1"), "kvscale_zero": ("kv_scale", 0.0),
  "mask_grad": ("tree_mask", torch.ones(3, 3, requires_grad=True)), "mask_list": ("tree_mask", [[True]]), "mask_int32": ("tree_mask", lambda t: t.int()),
  "mask_meta": ("tree_mask", _meta), "mask_narrow": ("tree_mask", lambda t: t[:2, :2]), "mask_rect": ("tree_mask", lambda t: t.new_zeros(4, 3)),
  "words_batch": ("tree_mask", lambda t: torch.zeros(5, 3, dtype=torch.int64, device=t.device)),
}


def _layout_chain(layout):
  return ["bt_int64", "bt_nopages", "cache_page32", "bt_meta"] if layout == "paged" else ["cache_batch", "cache_cap100"]


def check_order(func, layout):
  """The faults of ``func``'s checks in the order the parent makes the checks: one fault per check (a check with alternatives — cache_seqlens as an int, a tensor
  or neither — stands with one of them; the others are single-fault rows only)."""
  ragged, fp8, tree = func in RAGGED, func.endswith("_fp8"), func.endswith("_tree")
  head = ["unserved"] + (["kvscale_str"] if fp8 else []) + ["scale_missing", "scale_str"]
  dims = ["q_f32", "q_rank", "cache_dim", "hdv_float", "hdv_100", "hdv_256", "cache_heads", "splits_neg", "cache_meta"]
  kv = ["kv_dtype", "kv_meta", "kv_heads", "kv_stride"]
  if ragged:
    chain = head + ["q_list", "cache_none", "cu_list", "lens_list", "kv_list", "q_grad", "cache_grad", "kv_grad"] + dims + [
      "cu_int64", "cu_rank", "max_neg", "lens_int64", "lens_short"] + _layout_chain(layout) + kv
  else:
    chain = head + ["q_list", "q_grad", "cache_none", "cache_grad", "kv_list", "kv_grad"] + dims + _layout_chain(layout) + ["lens_int64"] + kv
  if tree:
    chain += ["mask_grad", "mask_int32", "max_65" if ragged else "q_sq65", "mask_meta", "mask_narrow"]
  return chain


def single_faults(func, layout):
  ragged, fp8, tree = func in RAGGED, func.endswith("_fp8"), func.endswith("_tree")
  more = ["lens_str"] + ([] if ragged else ["lens_neg"])
  if fp8:
    more += ["kvscale_tensor", "kvscale_zero", "cache_16bit"]
  if tree:
    more += ["mask_list", "mask_rect", "words_batch"]
  return check_order(func, layout) + more


def combine(f1, f2):
  """Whether two faults can stand in one call: on different arguments, or two transforms of one tensor."""
  (k1, v1), (k2, v2) = FAULTS[f1], FAULTS[f2]
  return k1 != k2 or (callable(v1) and callable(v2))


def apply_faults(a, faults):
  for name in faults:
    key, v = FAULTS[name]
    if v is _POP:
      a.pop(key)
    elif callable(v):
      a[key] = v(a[key])
    else:
      a[key] = v
  return a


def refusal_rows():
  """[(func, layout, [faults])]: every single fault, then every combinable pair of neighbours of the check order, then the pair that tells the uniform checker's
  per-tensor interleaving of the tensor test and the grad test from the ragged checker's two loops."""
  rows = []
  for func in FUNCS:
    for layout in ("paged", "contig"):
      rows += [(func, layout, [f]) for f in single_faults(func, layout)]
      chain = check_order(func, layout)
      pairs = [(f1, f2) for f1, f2 in zip(chain, chain[1:]) if combine(f1, f2)] + [("q_grad", "cache_none"), ("cache_grad", "kv_list")]
      rows += [(func, layout, list(p)) for p in dict.fromkeys(pairs)]
  return rows


def _applicable(func, faults):
  """float8 tensors cannot require grad: that fault has no FP8 row."""
  return not (func.endswith("_fp8") and "cache_grad" in faults)


# ----------------------------------------------------------------------------------------------------------------------------- replay
def run_refusal(row):
  """-> ([type name, message], the exception)."""
  a = apply_faults(base_args(row["func"], row["layout"]), row["faults"])
  try:
    getattr(_kvcache(), row["func"])(**a)
  except Exception as e:  # noqa: BLE001 (whatever is raised is what is recorded)
    return [type(e).__name__, str(e)], e
  return ["returned", ""], None


_SHORT = {torch.bfloat16: "bf16", torch.float16: "f16", torch.float32: "f32", torch.int32: "i32", torch.int64: "i64", torch.float8_e4m3fn: "e4m3"}


def _tensor(t, who):
  return f"{who}:{_SHORT[t.dtype]}{list(t.shape)}({','.join(map(str, t.stride()))})@{t.device.type}".replace(" ", "")


class _Ops(TorchDispatchMode):
  """Every ``ffpa_attn::*`` op of the block as one string, ``name(argument=value, ...)`` in the schema's names: a tensor as ``who:dtype[shape](strides)@device``,
  anything else as ``repr:type``."""

  def __init__(self, caller_args):
    super().__init__()
    self.caller, self.ops = caller_args, []

  def _arg(self, v):
    if isinstance(v, torch.Tensor):
      return _tensor(v, next((k for k, t in self.caller.items() if t is v), "new"))
    return f"{v!r}:{type(v).__name__}"

  def __torch_dispatch__(self, func, types, args=(), kwargs=None):
    kwargs = kwargs or {}
    if func._schema.name.startswith("ffpa_attn::"):
      named = list(zip((x.name for x in func._schema.arguments), args)) + list(kwargs.items())
      self.ops.append(f"{func._schema.name}({', '.join(f'{n}={self._arg(v)}' for n, v in named)})")
    return func(*args, **kwargs)


def run_served(row):
  a = base_args(row["func"], row["layout"], row["dtype"], "meta", row["kv"], row["lens"] or "tensor", row["mask"] or "bool2", row["empty"])
  if row["causal"] is not None:
    a["causal"] = row["causal"]
  a["return_softmax_lse"] = row["lse"]
  if row["splits"]:
    a["num_splits"] = row["splits"]
  with _Ops(a) as rec:
    out = getattr(_kvcache(), row["func"])(**a)
  outs = list(out) if isinstance(out, tuple) else [out]
  return {"ops": rec.ops, "returns": [_tensor(t, "out") for t in outs]}


def served_rows():
  """Per function: (1) what shapes the call — {paged, contiguous} x {no kv, kv, kv with Snew = 0 in the uniform calls} x {cache_seqlens a tensor, an int in the uniform
  calls} fully crossed, and {paged, contiguous} x {the tree mask as bool [W, W], bool [B, W, W], packed words} — bf16, not causal, no LSE; (2) what does not — {bf16, fp16 with num_splits = 2: a default num_splits
  does not reach the op's arguments} x {causal off, on where the call has it} x {LSE off, on} — fully crossed on the paged call with kv; (3) the empty batches, with
  a tree mask of a wrong dtype: an empty batch never looks at its mask."""
  rows = []
  for func in FUNCS:
    ragged, tree = func in RAGGED, func.endswith("_tree")
    row = lambda **kw: {**dict(func=func, layout="paged", dtype="bf16", kv="given", lse=False, causal=None if tree else False, lens=None if ragged else "tensor",
                               mask="bool2" if tree else None, splits=0, empty=None), **kw}
    shaping = dict(layout=("paged", "contig"), kv=("none", "given") if ragged else ("none", "given", "empty"), lens=(None,) if ragged else ("tensor", "int"))
    rows += [row(**dict(zip(shaping, v))) for v in itertools.product(*shaping.values())]
    rows += [row(layout=layout, mask=mask) for layout in ("paged", "contig") for mask in ("bool3", "words") if tree]
    flags = dict(dtype=("bf16", "fp16"), causal=(None,) if tree else (False, True), lse=(False, True))
    rows += [row(**dict(zip(flags, v)), splits=2 if v[0] == "fp16" else 0) for v in itertools.product(*flags.values()) if v != ("bf16", row()["causal"], False)]
    for layout, empty, lse in itertools.product(("paged", "contig"), ("T0",) if ragged else ("B0", "Sq0"), (False, True)):
      rows.append(row(layout=layout, lse=lse, mask="int32" if tree else None, empty=empty))
  return rows


def signatures():
  kv = _kvcache()
  return {f: {"signature": re.sub(r" at 0x[0-9a-fA-F]+", " at 0x", str(inspect.signature(getattr(kv, f)))), "doc": getattr(kv, f).__doc__} for f in FUNCS}


def replay(kind, row):
  """What the working tree answers to one row of the list: compare with ``row["want"]``."""
  return run_refusal(row)[0] if kind == "refusals" else run_served(row)


# The file holds every row, packed: rows that answer alike are one entry.  A refusal's message stands with ``{name}`` for the function's name, under the (function,
# layout) pairs that give it ("0p" = FUNCS[0], paged); a two-fault row says WHICH of its two faults' own answers it gives (0 or 1), not the answer again.  A served
# entry lists the rows — their option values in _SERVED_KEYS' order — in front of the one answer, its op calls as indices into "ops".
_SERVED_KEYS = ("layout", "dtype", "kv", "lse", "causal", "lens", "mask", "splits", "empty")


def _at(row):
  return f"{FUNCS.index(row['func'])}{row['layout'][0]}"


def pack(rec):
  single = {(r["func"], r["layout"], r["faults"][0]): r["want"] for r in rec["refusals"] if len(r["faults"]) == 1}
  refusals = {}
  for r in rec["refusals"]:
    if len(r["faults"]) == 1:
      key = (tuple(r["faults"]), r["want"][0], r["want"][1].replace(r["func"], "{name}"))
    else:
      key = (tuple(r["faults"]), [single[r["func"], r["layout"], f] for f in r["faults"]].index(r["want"]))
    refusals.setdefault(key, []).append(_at(r))
  served = {}
  for r in rec["served"]:
    served.setdefault((r["func"], json.dumps(r["want"])), []).append([r[k] for k in _SERVED_KEYS])
  ops = list(dict.fromkeys(op for r in rec["served"] for op in r["want"]["ops"]))  # (an op call that several rows make stands once; the entries hold its index)
  entries = [{"func": f, "rows": rows, **json.loads(want)} for (f, want), rows in served.items()]
  return {"signatures": rec["signatures"],
          "refusals": [{"faults": list(k[0]), **({"want": list(k[1:])} if len(k) == 3 else {"says": k[1]}), "at": " ".join(at)} for k, at in refusals.items()],
          "ops": ops, "served": [{**e, "ops": [ops.index(op) for op in e["ops"]]} for e in entries]}


def unpack(packed):
  refusals, single = [], {}
  for e in sorted(packed["refusals"], key=lambda e: "says" in e):  # (the single faults first: a two-fault entry points at their answers)
    for at in e["at"].split():
      func, layout = FUNCS[int(at[0])], {"p": "paged", "c": "contig"}[at[1]]
      if "want" in e:
        want = single[func, layout, e["faults"][0]] = [e["want"][0], e["want"][1].replace("{name}", func)]
      else:
        want = single[func, layout, e["faults"][e["says"]]]
      refusals.append({"func": func, "layout": layout, "faults": e["faults"], "want": want})
  served = [{"func": e["func"], **dict(zip(_SERVED_KEYS, row)), "want": {"ops": [packed["ops"][i] for i in e["ops"]], "returns": e["returns"]}}
            for e in packed["served"] for row in e["rows"]]
  return {"signatures": packed["signatures"], "refusals": refusals, "served": served}


def load(path=OUT):
  """The rows of the file, unpacked: ``{"signatures", "refusals": [row + "want"], "served": [row + "want"]}``."""
  with open(path, encoding="utf-8") as f:
    return unpack(json.load(f))


# ----------------------------------------------------------------------------------------------------------------------------- coverage of the raise statements
def _checked_raises():
  """{(file, first line, last line)} of every ``raise`` in the functions whose refusals are recorded: the six entry points, every ``_mla_*`` helper of kvcache.py
  (the checkers and the dtype rule; the sparse call has none under that prefix), ``_tree_words``, and ``check_kv_scale`` of the binding."""
  from ffpa_attn_amd import hip

  found = set()
  for mod, want in ((_kvcache(), lambda n: n in FUNCS or n.startswith("_mla_") or n == "_tree_words"), (hip, lambda n: n == "check_kv_scale")):
    path = os.path.abspath(inspect.getsourcefile(mod))
    with open(path, encoding="utf-8") as f:
      tree = ast.parse(f.read())
    for fn in tree.body:
      if isinstance(fn, ast.FunctionDef) and want(fn.name):
        found |= {(path, n.lineno, n.end_lineno) for n in ast.walk(fn) if isinstance(n, ast.Raise)}
  return found


def _raise_site(exc, raises):
  """The checked ``raise`` the exception came from: the innermost traceback frame that stands on one."""
  site = None
  for frame, line in traceback.walk_tb(exc.__traceback__):
    path = os.path.abspath(frame.f_code.co_filename)
    site = next((r for r in raises if r[0] == path and r[1] <= line <= r[2]), site)
  return site


def record():
  raises = _checked_raises()
  hit, refusals = set(), []
  for func, layout, faults in refusal_rows():
    if not _applicable(func, faults):
      continue
    row = {"func": func, "layout": layout, "faults": faults}
    want, exc = run_refusal(row)
    assert exc is not None, f"{row} was served"
    site = _raise_site(exc, raises)
    assert site is not None, f"{row} ended outside the checked functions: {want}"
    if len(faults) == 1:
      hit.add(site)
    refusals.append({**row, "want": want})
  missed = sorted(raises - hit)
  assert not missed, f"no single-fault row ends on: {[(os.path.basename(p), a) for p, a, _ in missed]}"
  served = [{**row, "want": run_served(row)} for row in served_rows()]
  return {"signatures": signatures(), "refusals": refusals, "served": served}, len(raises)


def dump(rec, path):
  rec = pack(rec)
  lines = ["{", '"signatures": ' + json.dumps(rec["signatures"], ensure_ascii=False, indent=1) + ","]
  for kind in ("refusals", "ops", "served"):
    lines.append(f'"{kind}": [')
    lines += [json.dumps(r, ensure_ascii=False) + ("," if i + 1 < len(rec[kind]) else "") for i, r in enumerate(rec[kind])]
    lines.append("]" if kind == "served" else "],")
  lines.append("}")
  with open(path, "w", encoding="utf-8") as f:
    f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
  ap = argparse.ArgumentParser()
  ap.add_argument("--out", default=OUT)
  args = ap.parse_args()
  rec, n = record()
  dump(rec, args.out)
  print(f"{len(rec['refusals'])} refusals (every one of the {n} raise statements reached by a single fault), {len(rec['served'])} served calls -> {args.out}")
