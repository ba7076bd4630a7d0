"""Record tests/golden/kv_front_calls.json: what the Python front end of the 16-bit KV-cache family answers, call by call, WITHOUT a device.

    PYTHONPATH=<checkout> python tests/golden/make_kv_front_calls.py [--out PATH]

The six entry points (ffpa_attn_with_kvcache, _tree, _window, _softcap, _cascade and ffpa_attn_varlen_with_kvcache) are recorded the three ways
make_mla_front_calls.py records the latent family, with its helpers and its conventions:

* signatures: ``str(inspect.signature(f))`` and ``f.__doc__`` — the docstring as its sha256: the six texts are 18 kB that kvcache.py holds already;
* refusals: a smallest valid argument set on CPU tensors (new keys, rotary tables and — ragged — positions given, so that every check is awake), one named fault
  (or two, for the ORDER of neighbouring checks) applied to it, and the exception's type name and full message.  The recorder proves its own coverage: it finds
  every ``raise`` of the checked functions — the entry points and every function of kvcache.py they reach, by name, through calls — with ``ast`` and asserts that
  a single-fault row ended on each of them; UNREACHABLE names the ones no argument set of these calls can reach, with the reason;
* served calls: argument sets on META tensors under a ``TorchDispatchMode`` -> the sequence of ``ffpa_attn::*`` ops with every argument (a tensor as
  ``who:dtype[shape](strides)@device``, ``who`` the caller's argument it IS — Python identity — or ``new``; anything else as ``repr:type``), the torch ops that
  give a launch argument its VALUE (arange, full, zeros, sub, clamp: the boundaries and lengths a meta tensor does not show), and the returned tensors.  The
  contiguous plain launches call ``hip.varlen_forward`` directly: the recorder swaps it for a stub that records the call — bound to the real signature, defaults
  applied: every parameter as the function receives it — and returns meta outputs of its shapes.

tests/test_kvcache_front.py replays every row through ``replay`` and compares for equality.  The committed list was recorded from the commit BEFORE the front
end was folded into one checker and one step: signatures, docstrings, order and wording of every refusal and every launch argument are pinned to that."""

import argparse
import ast
import hashlib
import importlib.util
import inspect
import itertools
import json
import os
import re

import torch
from torch.utils._python_dispatch import TorchDispatchMode

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "kv_front_calls.json")

_spec = importlib.util.spec_from_file_location("make_mla_front_calls", os.path.join(HERE, "make_mla_front_calls.py"))
mla = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mla)
_meta, _grad, _strided, _other16, _tensor, _raise_site, _kvcache, _DTYPES = (mla._meta, mla._grad, mla._strided, mla._other16, mla._tensor, mla._raise_site,
                                                                              mla._kvcache, mla._DTYPES)

PLAIN, TREE, WINDOW, SOFTCAP, CASCADE, VARLEN = FUNCS = (
  "ffpa_attn_with_kvcache", "ffpa_attn_with_kvcache_tree", "ffpa_attn_with_kvcache_window", "ffpa_attn_with_kvcache_softcap", "ffpa_attn_with_kvcache_cascade",
  "ffpa_attn_varlen_with_kvcache")

# "small": the shape of every row but the cascade rule's; "big": a shape on which cascade_rule says yes at P = 8192 and no at P = 8128 (meta tensors: no memory)
SHAPES = {"small": dict(B=2, Sq=3, Hq=4, Hkv=2, D=64, pages=4, page=64, per_seq=2), "big": dict(B=65, Sq=1, Hq=4, Hkv=1, D=512, pages=4, page=64, per_seq=256)}
RAGGED_LENS = (1, 0, 3)
ROTARY_HALF = 16  # rotary_dim = 32
# what a call takes besides the family's common arguments, at a valid value
OWN = {PLAIN: {}, TREE: {}, WINDOW: {"window_size": (4, 0)}, SOFTCAP: {"softcap": 30.0}, CASCADE: {"shared_prefix_len": 64, "cascade": True}, VARLEN: {}}


# ----------------------------------------------------------------------------------------------------------------------------- the argument sets
def base_args(func, layout="paged", dtype="bf16", device="cpu", kv="given", rotary=True, lens="tensor", positions=True, mask="bool2", empty=None, shape="small"):
  """A smallest valid keyword set of ``func``.  ``kv``: "none" | "given" | "empty" (Snew = 0, uniform calls); ``rotary``: the tables, with ``kv``; ``lens``:
  cache_seqlens "none" | "int" | "tensor" (uniform calls); ``positions``: with the tables, ragged call; ``mask``: "bool2" [Sq, Sq] | "bool3" [B, Sq, Sq] | "words"
  int64 [B, Sq]; ``empty``: None | "B0" | "Sq0" (uniform) | "T0" (ragged)."""
  s = SHAPES[shape]
  Hq, Hkv, D = s["Hq"], s["Hkv"], s["D"]
  cap = s["page"] * s["per_seq"]
  dt = _DTYPES[dtype]

  def z(*shape, dtype=dt):
    return torch.zeros(*shape, dtype=dtype, device=device)

  if func == VARLEN:
    seqs = (0, 0, 0) if empty == "T0" else RAGGED_LENS
    B, T = len(seqs), sum(seqs)
    a = {"q": z(T, Hq, D)}
    new_shape = (T, Hkv, D)
  else:
    B, Sq = (0 if empty == "B0" else s["B"]), (0 if empty == "Sq0" else s["Sq"])
    a = {"q": z(B, Sq, Hq, D)}
    new_shape = (B, 0 if kv == "empty" else s["Sq"], Hkv, D)
  for name in ("k_cache", "v_cache"):
    a[name] = z(s["pages"], s["page"], Hkv, D) if layout == "paged" else z(B, cap, Hkv, D)
  if func == VARLEN:
    a["cu_seqlens_q"] = torch.tensor([0, *itertools.accumulate(seqs)], dtype=torch.int32).to(device)
    a["max_seqlen_q"] = max(seqs)
    a["cache_seqlens"] = z(B, dtype=torch.int32)
  elif lens != "none":
    a["cache_seqlens"] = 5 if lens == "int" else z(B, dtype=torch.int32)
  if layout == "paged":
    a["block_table"] = z(B, s["per_seq"], dtype=torch.int32)
  if kv != "none":
    a["k"], a["v"] = z(*new_shape), z(*new_shape)
    if rotary and func != TREE:
      a["rotary_cos"], a["rotary_sin"] = z(cap, ROTARY_HALF), z(cap, ROTARY_HALF)
      if positions and func == VARLEN:
        a["positions"] = z(new_shape[0], dtype=torch.int32)
  if func == TREE:
    n = a["q"].size(1)
    a["tree_mask"] = {"bool2": lambda: z(n, n, dtype=torch.bool), "bool3": lambda: z(B, n, n, dtype=torch.bool), "words": lambda: z(B, n, dtype=torch.int64)}[mask]()
  return {**a, **OWN[func]}


# ----------------------------------------------------------------------------------------------------------------------------- the faults
def _each(*keys):
  """A fault on several arguments at once: ``fn`` on each of them that is there and (still) a tensor."""
  def of(fn):
    def f(a):
      for k in keys:
        if isinstance(a.get(k), torch.Tensor):
          a[k] = fn(a[k])
    return f
  return of


_CACHES, _NEW, _TABLES = ("k_cache", "v_cache"), ("k", "v"), ("rotary_cos", "rotary_sin")
_ALL = "*"  # the argument of a fault that takes the whole argument set


def _per(prefix, key, faults):
  return {f"{prefix}_{n}": (key, v) for n, v in faults.items()}


# name -> (argument, a value that REPLACES it | a function that TRANSFORMS the tensor it holds), or (_ALL, a function of the argument set).  Two faults on one
# argument combine only if both transform.
FAULTS = {
  "batch_idx": ("cache_batch_idx", torch.zeros(2, dtype=torch.int32)), "leftpad": ("cache_leftpad", torch.zeros(2, dtype=torch.int32)),
  "alibi": ("alibi_slopes", torch.zeros(4)), "plain_window": ("window_size", (1, 1)), "plain_window_none": ("window_size", None), "plain_softcap": ("softcap", 1.0),
  "v_none": ("v", None), "k_none": ("k", None), "cos_none": ("rotary_cos", None), "sin_none": ("rotary_sin", None), "kv_none": (_ALL, lambda a: a.update(k=None, v=None)),
  "tables_none": (_ALL, lambda a: a.update(rotary_cos=None, rotary_sin=None)),
  **_per("q", "q", {"list": [1.0], "grad": _grad, "f32": lambda t: t.float(), "rank": lambda t: t[0], "dim": lambda t: t[..., :32], "heads": lambda t: t.narrow(-2, 0, 3),
                    "sq65": lambda t: torch.zeros(t.size(0), 65, *t.shape[2:], dtype=t.dtype), "sq0": lambda t: t[:, :0]}),
  **{f"{p}_{n}": (key, v) for p, key in (("kc", "k_cache"), ("vc", "v_cache"))
     for n, v in {"none": None, "grad": _grad, "dtype": _other16, "rank": lambda t: t[0], "meta": _meta}.items()},
  "vc_shape": ("v_cache", lambda t: t[:, :32]),
  "all_d12": (_ALL, _each("q", *_CACHES, *_NEW)(lambda t: t[..., :12])), "all_d0": (_ALL, _each("q", *_CACHES, *_NEW)(lambda t: t[..., :0])),
  "all_d1032": (_ALL, _each("q", *_CACHES, *_NEW)(lambda t: torch.zeros(*t.shape[:-1], 1032, dtype=t.dtype))),
  "heads0": (_ALL, _each(*_CACHES, *_NEW)(lambda t: t.narrow(-2, 0, 0))),
  "splits_neg": ("num_splits", -1), "splits_bool": ("num_splits", True), "splits_float": ("num_splits", 1.0),
  **_per("bt", "block_table", {"list": [[0, 1]], "int64": lambda t: t.long(), "rank": lambda t: t[0], "batch": lambda t: t[:1], "nopages": lambda t: t[:, :0], "meta": _meta}),
  "page32": (_ALL, _each(*_CACHES)(lambda t: t[:, :32])), "page0": (_ALL, _each(*_CACHES)(lambda t: t[:, :0])),
  "cache_batch": (_ALL, _each(*_CACHES)(lambda t: t[:1])),
  **_per("lens", "cache_seqlens", {"none": None, "neg": -1, "str": "5", "bool": True, "list": [0, 0], "int64": lambda t: t.long(), "rank": lambda t: t[None],
                                   "short": lambda t: t[:1], "meta": _meta}),
  **{f"{p}_{n}": (p, v) for p in _NEW
     for n, v in {"list": [1.0], "grad": _grad, "dtype": _other16, "meta": _meta, "rank": lambda t: t[0], "rows": lambda t: t[:1], "heads": lambda t: t.narrow(-2, 0, 1),
                  "dim": lambda t: t[..., :32], "stride": _strided}.items()},
  "v_snew": ("v", lambda t: t[:, :1]),
  **{f"{p}_{n}": (key, v) for p, key in (("cos", "rotary_cos"), ("sin", "rotary_sin"))
     for n, v in {"list": [1.0], "dtype": _other16, "meta": _meta, "rank": lambda t: t[None], "strided": _strided}.items()},
  "sin_cols": ("rotary_sin", lambda t: t[:, :8].contiguous()),
  "rot_dim0": (_ALL, _each(*_TABLES)(lambda t: t[:, :0])), "rot_dim8": (_ALL, _each(*_TABLES)(lambda t: t[:, :4].contiguous())),
  "rot_dim128": (_ALL, _each(*_TABLES)(lambda t: torch.zeros(t.size(0), 64, dtype=t.dtype))), "rot_rows": (_ALL, _each(*_TABLES)(lambda t: t[:64])),
  **_per("cu", "cu_seqlens_q", {"list": [0, 1, 1, 4], "int64": lambda t: t.long(), "rank": lambda t: t[None], "short": lambda t: t[:1],
                                "stride": lambda t: torch.zeros(2 * t.numel(), dtype=t.dtype)[::2], "meta": _meta}),
  "max_neg": ("max_seqlen_q", -1), "max_zero": ("max_seqlen_q", 0), "max_bool": ("max_seqlen_q", True), "max_float": ("max_seqlen_q", 3.0),
  **_per("pos", "positions", {"list": [0, 0, 0, 0], "int64": lambda t: t.long(), "rank": lambda t: t[None], "short": lambda t: t[:1],
                              "stride": lambda t: torch.zeros(2 * t.numel(), dtype=t.dtype)[::2], "meta": _meta}),
  **_per("win", "window_size", {"none": None, "int": 5, "triple": (1, 2, 3), "float": (1.0, 2), "bool": (True, 0), "neg": (-2, 0), "neg_right": (0, -2)}),
  **_per("cap", "softcap", {"str": "30", "bool": True, "none": None, "neg": -1.0, "nan": float("nan"), "inf": float("inf")}),
  **_per("mask", "tree_mask", {"grad": torch.ones(3, 3, requires_grad=True), "list": [[True]], "int32": lambda t: t.int(), "meta": _meta, "narrow": lambda t: t[:2, :2],
                               "rect": lambda t: t.new_zeros(4, 3), "rank": lambda t: t[0], "batch": lambda t: t.new_zeros(5, 3, 3)}),
  "words_batch": ("tree_mask", lambda t: torch.zeros(5, 3, dtype=torch.int64)), "words_rank": ("tree_mask", lambda t: torch.zeros(3, dtype=torch.int64)),
  "words_cols": ("tree_mask", lambda t: torch.zeros(1, 2, dtype=torch.int64)),
  **_per("P", "shared_prefix_len", {"float": 64.0, "bool": True, "neg": -64, "big": 192, "odd": 32, "big_odd": 160}),
  "cascade_str": ("cascade", "yes"), "cascade_int": ("cascade", 1),
}


def _new(ragged):
  per = lambda p: [f"{p}_list", f"{p}_dtype", f"{p}_meta", f"{p}_heads", f"{p}_stride"]
  return per("k") + per("v") if ragged else per("k")[:1] + ["k_grad"] + per("k")[1:] + per("v")[:1] + ["v_grad"] + per("v")[1:] + ["v_snew"]


_TABLE_CHAIN = ["cos_list", "cos_dtype", "cos_meta", "cos_rank", "sin_list", "sin_dtype", "sin_meta", "sin_rank", "sin_cols", "rot_dim8", "rot_rows"]
_DIMS = ["q_f32", "q_rank", "vc_shape", "q_dim", "all_d12", "q_heads", "splits_neg"]


def _layout_chain(layout):
  return ["bt_int64", "bt_nopages", "page32", "bt_meta"] if layout == "paged" else ["cache_batch"]


def check_order(func, layout):
  """The faults of ``func``'s checks in the order the parent makes the checks: one fault per check (a check with alternatives stands with one of them; the
  others are single-fault rows only).  The entry point's own arguments stand where it tests them: in front of the cache checks or — the cascade's P against
  the capacity and the page, the tree mask — behind them."""
  if func == VARLEN:
    return ["cap_neg", "win_neg", "v_none", "q_list", "kc_none", "vc_none", "cu_list", "lens_list", "q_grad", "kc_grad", "vc_grad", "k_grad", "v_grad"] + _DIMS + [
      "cu_int64", "cu_rank", "max_neg", "lens_int64", "lens_short"] + _layout_chain(layout) + ["kc_meta"] + _new(True) + _TABLE_CHAIN + ["pos_int64", "pos_short"]
  own = {PLAIN: ["batch_idx"], TREE: [], WINDOW: ["win_neg"], SOFTCAP: ["cap_neg", "win_neg"], CASCADE: ["P_float", "P_neg", "cascade_str"]}[func]
  chain = own + ["v_none", "q_list", "q_grad", "kc_none", "kc_grad", "vc_none", "vc_grad"] + _DIMS + _layout_chain(layout) + ["kc_meta", "lens_int64", "lens_none"] + _new(False)
  if func == TREE:
    return chain + ["mask_grad", "mask_int32", "q_sq65", "mask_meta", "mask_narrow"]
  return chain + _TABLE_CHAIN + (["P_big", "P_odd"] if func == CASCADE and layout == "paged" else ["P_big"] if func == CASCADE else [])


def single_faults(func, layout):
  more = ["k_none", "kv_none", "sin_none", "cos_none", "kc_dtype", "vc_dtype", "kc_rank", "vc_rank", "vc_meta", "all_d0", "all_d1032", "heads0", "splits_bool",
          "splits_float", "lens_str", "lens_meta", "lens_rank", "k_rank", "k_dim", "v_rank", "v_dim", "cos_strided", "sin_strided", "rot_dim0", "rot_dim128"]
  more += ["bt_list", "bt_rank", "bt_batch", "page0"] if layout == "paged" else []
  if func == VARLEN:
    more += ["k_rows", "v_rows", "tables_none", "cu_short", "cu_stride", "cu_meta", "max_zero", "max_bool", "max_float", "pos_list", "pos_rank", "pos_stride", "pos_meta"]
  else:
    more += ["lens_neg", "lens_bool", "lens_list"]
  if func == PLAIN:
    more += ["leftpad", "alibi", "plain_window", "plain_window_none", "plain_softcap"]
  if func in (WINDOW, SOFTCAP, VARLEN):
    more += ["win_none", "win_int", "win_triple", "win_float", "win_bool", "win_neg_right"]
  if func in (SOFTCAP, VARLEN):
    more += ["cap_str", "cap_bool", "cap_none", "cap_nan", "cap_inf"]
  if func == TREE:
    more = [f for f in more if f.split("_")[0] not in ("cos", "sin", "rot") and f != "kv_none"] + ["q_sq0", "mask_list", "mask_rect", "mask_rank", "mask_batch", "words_batch", "words_rank", "words_cols"]
  if func == CASCADE:
    more += ["P_bool", "cascade_int"] + (["P_big_odd"] if layout == "paged" else [])
  return check_order(func, layout) + more


def combine(f1, f2):
  """Whether two faults can stand in one call: on different arguments, or two transforms (the faults on the whole argument set transform what is a tensor)."""
  (k1, v1), (k2, v2) = FAULTS[f1], FAULTS[f2]
  return (k1 != k2 and _ALL not in (k1, k2)) or (callable(v1) and callable(v2))


def apply_faults(a, faults):
  for name in faults:
    key, v = FAULTS[name]
    if key == _ALL:
      v(a)
    elif callable(v):
      a[key] = v(a[key])
    else:
      a[key] = v
  return a


def _applicable(func, layout, faults):
  """A fault on an argument the call does not take (the tree call's rotary tables) has no row."""
  a = base_args(func, layout)
  return all(FAULTS[f][0] in (_ALL, *a) or FAULTS[f][0] in inspect.signature(getattr(_kvcache(), func)).parameters for f in faults)


def refusal_rows():
  """[(func, layout, [faults])]: every single fault, then every combinable pair of neighbours of the check order, then the pairs that tell the uniform checker's
  per-tensor interleaving of the tensor test and the grad test from the ragged checker's two loops."""
  rows = []
  for func in FUNCS:
    for layout in ("paged", "contig"):
      rows += [(func, layout, [f]) for f in dict.fromkeys(single_faults(func, layout))]
      chain = check_order(func, layout)
      pairs = [(f1, f2) for f1, f2 in zip(chain, chain[1:]) if combine(f1, f2)] + [("q_grad", "kc_none"), ("kc_grad", "vc_none"), ("vc_grad", "k_list"), ("k_grad", "v_list")]
      rows += [(func, layout, list(p)) for p in dict.fromkeys(pairs)]
  return [r for r in rows if _applicable(*r)]


# ----------------------------------------------------------------------------------------------------------------------------- replay
def run_refusal(row):
  """-> ([type name, message], the exception)."""
  a = apply_faults(base_args(row["func"], row["layout"]), row["faults"])
  try:
    getattr(_kvcache(), row["func"])(**a)
  except Exception as e:  # noqa: BLE001 (whatever is raised is what is recorded)
    return [type(e).__name__, str(e)], e
  return ["returned", ""], None


_VALUE_OPS = ("aten::arange", "aten::full", "aten::zeros", "aten::sub", "aten::clamp")


class _Ops(TorchDispatchMode):
  """Every ``ffpa_attn::*`` op of the block — and every torch op of _VALUE_OPS, every ``hip.varlen_forward`` call — as one string, ``name(argument=value, ...)`` in
  the schema's names: a tensor as ``who:dtype[shape](strides)@device``, anything else as ``repr:type``."""

  def __init__(self, caller_args):
    super().__init__()
    self.caller, self.ops = caller_args, []

  def _arg(self, v):
    if isinstance(v, torch.Tensor):
      return _tensor(v, next((k for k, t in self.caller.items() if t is v), "new"))
    return f"{v!r}:{type(v).__name__}"

  def _add(self, name, named):
    self.ops.append(f"{name}({', '.join(f'{n}={self._arg(v)}' for n, v in named)})")

  def __torch_dispatch__(self, func, types, args=(), kwargs=None):
    kwargs = kwargs or {}
    if func._schema.name.startswith("ffpa_attn::") or func._schema.name in _VALUE_OPS:
      self._add(func._schema.name, list(zip((x.name for x in func._schema.arguments), args)) + list(kwargs.items()))
    return func(*args, **kwargs)

  def varlen_forward(self, real):
    """The stand-in of ``hip.varlen_forward``: the call as a row, meta outputs of the real function's shapes."""
    sig = inspect.signature(real)

    def stub(*args, **kwargs):
      bound = sig.bind(*args, **kwargs)
      bound.apply_defaults()
      self._add("hip.varlen_forward", bound.arguments.items())
      q = bound.arguments["q"]
      return q.new_empty(q.shape), (q.new_empty((q.size(1), q.size(0)), dtype=torch.float32) if bound.arguments["return_lse"] else None)

    return stub


def served_args(row):
  a = base_args(row["func"], row["layout"], row["dtype"], "meta", row["kv"], row["rotary"], row["lens"], row["positions"], row["mask"], row["empty"], row["shape"])
  a.update({k: tuple(v) if isinstance(v, list) else v for k, v in row["opts"].items()})
  return a


def run_served(row):
  from ffpa_attn_amd import hip

  a = served_args(row)
  real = hip.varlen_forward
  with _Ops(a) as rec:
    hip.varlen_forward = rec.varlen_forward(real)
    try:
      out = getattr(_kvcache(), row["func"])(**a)
    finally:
      hip.varlen_forward = real
  outs = list(out) if isinstance(out, tuple) else [out]
  return {"ops": rec.ops, "returns": [_tensor(t, "out") for t in outs]}


def served_rows():
  """Per function: (1) what shapes the call — {paged, contiguous} x {no k / v; k / v, Snew = 0 in the uniform calls: each without and with the rotary tables, and
  — ragged — positions} x {cache_seqlens none without k / v, a tensor; an int in the plain call: the checker that makes the lengths of it was one function for the
  five uniform calls before the fold too} fully crossed; (2) the flags — {causal} x {LSE} on both layouts, the paged rows in bf16, the contiguous ones in fp16 with
  num_splits = 2, a softmax scale and NeoX pairs; (3) the empty batches; (4) every branch of the launch choice: the window (-1, -1), a softcap of 0 (an int
  and a float) and a softcap under a window, the three forms of the tree mask, the ragged call's four launches; (5) the cascade under False / True / None, on
  either side of cascade_rule, at P = 0 and P = the capacity."""
  rows = []
  for func in FUNCS:
    ragged, tree = func == VARLEN, func == TREE
    row = lambda **kw: {**dict(func=func, layout="paged", dtype="bf16", kv="given", rotary=not tree, lens="tensor", positions=False, mask="bool2", empty=None,
                               shape="small", opts={}), **kw}
    for layout, kv in itertools.product(("paged", "contig"), ("none", "given") if ragged else ("none", "given", "empty")):
      for rotary, positions in [(False, False)] if kv == "none" or tree else [(False, False), (True, False), (True, True)] if ragged else [(False, False), (True, False)]:
        for lens in [x for x in ("none", "int", "tensor") if x == "tensor" or (x == "none" and kv == "none" and not ragged) or (x == "int" and func == PLAIN)]:
          rows.append(row(layout=layout, kv=kv, rotary=rotary, positions=positions, lens=lens))
    flags = dict(layout=("paged", "contig"), causal=(None,) if tree else (False, True), lse=(False, True))
    for layout, causal, lse in itertools.product(*flags.values()):
      dtype = "bf16" if layout == "paged" else "fp16"
      opts = {"return_softmax_lse": lse, **({} if causal is None else {"causal": causal})}
      if dtype == "fp16":
        opts.update({"num_splits": 2, "softmax_scale": 0.25}, **({} if tree else {"rotary_interleaved": False}))
      rows.append(row(layout=layout, dtype=dtype, opts=opts))
    for layout, empty, lse in itertools.product(("paged", "contig"), ("T0",) if ragged else ("B0",) if tree else ("B0", "Sq0"), (False, True)):
      rows.append(row(layout=layout, empty=empty, opts={"return_softmax_lse": lse}))
    for layout in ("paged", "contig"):
      choices = {PLAIN: [], TREE: [], CASCADE: [],
                 WINDOW: [{"window_size": [-1, -1]}, {"window_size": [-1, 0], "causal": True}, {"window_size": [1 << 40, 7]}],
                 SOFTCAP: [{"softcap": 0}, {"softcap": 0.0, "window_size": [4, 0]}, {"softcap": 30, "window_size": [4, 0], "causal": True}],
                 VARLEN: [{"window_size": [-1, -1]}, {"window_size": [4, 0]}, {"softcap": 30.0}, {"softcap": 30.0, "window_size": [4, 0]}, {"softcap": 0, "window_size": [-1, 0]},
                          {"softcap": 30.0, "return_softmax_lse": True, "causal": True}, {"window_size": [4, 0], "return_softmax_lse": True, "causal": True}]}[func]
      rows += [row(layout=layout, opts=o) for o in choices]
      rows += [row(layout=layout, mask=m, kv=kv) for m in ("bool3", "words") for kv in ("none", "given") if tree]
      if func == CASCADE:
        rows += [row(layout=layout, opts={"cascade": c, "return_softmax_lse": lse, "causal": lse}) for c in (False, None) for lse in (False, True)]
        rows += [row(layout=layout, opts={"shared_prefix_len": p}, kv=kv) for p in (0, 128) for kv in ("none", "given")]
        rows += [row(layout=layout, shape="big", kv=kv, opts={"shared_prefix_len": p, "cascade": c}) for p in (8128, 8192) for c in (None, True) for kv in ("none", "given")
                 if kv == "none" or (p, c) == (8192, None)]
  return rows


def signatures():
  kv = _kvcache()
  return {f: {"signature": str(inspect.signature(getattr(kv, f))), "doc_sha256": hashlib.sha256(getattr(kv, f).__doc__.encode()).hexdigest()} for f in FUNCS}


def replay(kind, row):
  """What the working tree answers to one row of the list: compare with ``row["want"]``."""
  return run_refusal(row)[0] if kind == "refusals" else run_served(row)


# The file holds every row, packed.  A refusal entry is one (faults, answer) under the (function, layout) pairs that give it ("0p" = FUNCS[0], paged); a two-fault
# entry says WHICH of its two faults' own answers it gives (0 or 1) where it gives one of them.  A served entry lists the rows that answer alike — each as what
# it changes of _ROW — behind the function's index in FUNCS and in front of the one answer: its calls as indices into "ops" — a call there is its name and its
# arguments, all as indices into "args" — and its returns as indices into "args".  A message stands with ``{name}`` for the name the function's checker speaks under.
_ROW = dict(layout="paged", dtype="bf16", kv="given", rotary=True, lens="tensor", positions=False, mask="bool2", empty=None, shape="small", opts={})
_ARG = re.compile(r", (?=\w+=)")


def _spoken(func):
  return VARLEN if func == VARLEN else PLAIN


def pack(rec):
  single = {(r["func"], r["layout"], r["faults"][0]): r["want"] for r in rec["refusals"] if len(r["faults"]) == 1}
  refusals = {}
  for r in rec["refusals"]:
    own = [single.get((r["func"], r["layout"], f)) for f in r["faults"]]
    key = (tuple(r["faults"]), own.index(r["want"])) if len(own) == 2 and r["want"] in own else (tuple(r["faults"]), r["want"][0], r["want"][1].replace(_spoken(r["func"]), "{name}"))
    refusals.setdefault(key, []).append(f"{FUNCS.index(r['func'])}{r['layout'][0]}")
  calls = list(dict.fromkeys(op for r in rec["served"] for op in r["want"]["ops"]))
  split = [(op[:op.index("(")], _ARG.split(op[op.index("(") + 1:-1])) for op in calls]
  args = list(dict.fromkeys([a for name, pieces in split for a in (name, *pieces)] + [t for r in rec["served"] for t in r["want"]["returns"]]))
  served = {}
  for r in rec["served"]:
    row = {k: v for k, v in r.items() if k not in ("func", "want") and v != {**_ROW, "rotary": r["func"] != TREE}[k]}
    served.setdefault((r["func"], json.dumps(r["want"])), []).append(row)
  return {"signatures": rec["signatures"],
          "refusals": [{"faults": list(k[0]), **({"says": k[1]} if len(k) == 2 else {"want": list(k[1:])}), "at": " ".join(at)} for k, at in refusals.items()],
          "args": args, "ops": [[args.index(a) for a in (name, *pieces)] for name, pieces in split],
          "served": [[FUNCS.index(f), rows, [calls.index(op) for op in json.loads(want)["ops"]], [args.index(t) for t in json.loads(want)["returns"]]]
                     for (f, want), rows in served.items()]}


def unpack(packed):
  refusals, single = [], {}
  for e in sorted(packed["refusals"], key=lambda e: "says" in e):  # (the single faults first: a two-fault entry may point at their answers)
    for at in e["at"].split():
      func, layout = FUNCS[int(at[0])], {"p": "paged", "c": "contig"}[at[1]]
      want = [e["want"][0], e["want"][1].replace("{name}", _spoken(func))] if "want" in e else single[func, layout, e["faults"][e["says"]]]
      if len(e["faults"]) == 1:
        single[func, layout, e["faults"][0]] = want
      refusals.append({"func": func, "layout": layout, "faults": e["faults"], "want": want})
  ops = [f"{packed['args'][name]}({', '.join(packed['args'][i] for i in pieces)})" for name, *pieces in packed["ops"]]
  served = [{"func": FUNCS[f], **_ROW, "rotary": FUNCS[f] != TREE, **row, "want": {"ops": [ops[i] for i in calls], "returns": [packed["args"][i] for i in returns]}}
            for f, rows, calls, returns in packed["served"] for row in rows]
  return {"signatures": packed["signatures"], "refusals": refusals, "served": served}


def load(path=OUT):
  """The rows of the file, unpacked: ``{"signatures", "refusals": [row + "want"], "served": [row + "want"]}``."""
  with open(path, encoding="utf-8") as f:
    return unpack(json.load(f))


# ----------------------------------------------------------------------------------------------------------------------------- coverage of the raise statements
# A ``raise`` of the checked functions that no argument set of these six calls reaches: a piece of its source text -> why.
UNREACHABLE = {
  "tree_mask must be bool [W, W]": "_tree_words' ``wide`` form is the latent tree calls' (their recorder reaches it); ffpa_attn_with_kvcache_tree never asks for it",
}
# pack_tree_mask is a public function with refusals of its own: _tree_words, its only caller here, has refused everything it would refuse.
_NOT_CHECKED = ("pack_tree_mask",)


def _checked_raises():
  """-> ({(file, first line, last line)} of every ``raise`` in the six entry points and in every function of kvcache.py they reach through calls by name,
  {those of UNREACHABLE})."""
  path = os.path.abspath(inspect.getsourcefile(_kvcache()))
  with open(path, encoding="utf-8") as f:
    source = f.read()
  funcs = {fn.name: fn for fn in ast.parse(source).body if isinstance(fn, ast.FunctionDef)}
  todo, seen = list(FUNCS), set()
  while todo:
    name = todo.pop()
    if name in seen or name in _NOT_CHECKED:
      continue
    seen.add(name)
    todo += [n.func.id for n in ast.walk(funcs[name]) if isinstance(n, ast.Call) and isinstance(n.func, ast.Name) and n.func.id in funcs]
  raises = [n for name in seen for n in ast.walk(funcs[name]) if isinstance(n, ast.Raise)]
  unreachable = set()
  for text in UNREACHABLE:
    sites = [n for n in raises if text in ast.get_source_segment(source, n)]
    assert len(sites) == 1, f"UNREACHABLE names {len(sites)} raise statements with {text!r}"
    unreachable.add((path, sites[0].lineno, sites[0].end_lineno))
  return {(path, n.lineno, n.end_lineno) for n in raises}, unreachable


def record():
  raises, unreachable = _checked_raises()
  hit, refusals = set(), []
  for func, layout, faults in refusal_rows():
    row = {"func": func, "layout": layout, "faults": faults}
    want, exc = run_refusal(row)
    assert exc is not None, f"{row} was served"
    site = _raise_site(exc, raises)
    assert site is not None, f"{row} ended outside the checked functions: {want}"
    if len(faults) == 1:
      hit.add(site)
    refusals.append({**row, "want": want})
  assert not hit & unreachable, "a raise listed as unreachable was reached"
  missed = sorted(raises - hit - unreachable)
  assert not missed, f"no single-fault row ends on: {[(os.path.basename(p), a) for p, a, _ in missed]}"
  served = [{**row, "want": run_served(row)} for row in served_rows()]
  return {"signatures": signatures(), "refusals": refusals, "served": served}, len(raises), len(unreachable)


def dump(rec, path):
  rec = pack(rec)
  lines = ["{", '"signatures": ' + json.dumps(rec["signatures"], ensure_ascii=False, indent=1) + ","]
  for kind in ("refusals", "args", "ops", "served"):
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
  rec, n, u = record()
  dump(rec, args.out)
  print(f"{len(rec['refusals'])} refusals (every one of the {n} raise statements but the {u} listed as unreachable reached by a single fault), "
        f"{len(rec['served'])} served calls -> {args.out}")
