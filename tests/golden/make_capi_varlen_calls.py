"""Record tests/golden/capi_varlen_calls.json: what the packed-call family of the C-ABI answers, call by call, WITHOUT a device.

    python tests/golden/make_capi_varlen_calls.py [--library PATH]

Run on a box without a GPU against the library whose behaviour is to be pinned (a host-layer refactor records it from the commit BEFORE the refactor and
replays it afterwards: tests/test_capi_varlen_families.py).  The plan queries read no tensor, so every pointer below is a made-up, suitably aligned address
and every shape is just integers.

The file is a list of calls, one per line.  A call has a ``form`` (one of FORMS: which exports it goes through and which structs it passes; a list of forms: one
call per form, all answered the same; a struct that a form does not take is not passed to it), field overrides for
the params and for the form's structs (over the form's defaults, ``defaults()`` below: fields neither names are zero, the q / k / v / o strides of a dense layout
and ``total_q`` = batch x max_seqlen_q unless named; a struct that is absent passes its defaults, ``null``: the struct pointer is NULL), ``cus`` (the FFPA_HIP_FAKE_CUS value; absent: unset) and ``null_out`` (the queries get NULL for out / buf /
slots).  ``got`` is what the library answered, in the short form of ``pack()``: ``plan`` = the five plan integers, or ``[status, ffpa_attn_last_error()]`` of a
refusal; ``kernel`` = the *_kernel string (a leading ``*``: ``kernel_stem()`` of the call, e.g. ``ffpa_fwd_m16_paged_tree_kernel``), ``ws`` = *_workspace_bytes (absent: 0), ``slots`` = *_compact_slots where the form has it, ``launch`` = ``[status,
text]`` of the launch export; ``"plan": "base"`` (calls that only the launch export refuses): every query answers what it answers the same call without its params overrides (the entry that
names no ``params``).  A query that refuses with the plan's status and text is left out, and so is a launch export that does what is expected of it
without a device: the plan's refusal again or, behind an accepted plan, NO_DEVICE.  ``unpack()`` restores the long form that ``replay()`` returns.
"""

from __future__ import annotations

import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "capi_varlen_calls.json")
ERR_NO_DEVICE = 9
NO_DEVICE = [ERR_NO_DEVICE, "no current HIP device"]  # what a launch export answers on a box without a device once every argument check has passed

# form -> (export stem, the structs behind params in argument order, takes a softcap float, has *_compact_slots)
FORMS = {
  "packed": ("ffpa_attn_varlen_fwd", (), False, False),
  "paged": ("ffpa_attn_varlen_paged_fwd", ("kv",), False, False),
  "tree": ("ffpa_attn_varlen_tree_fwd", ("kv", "tree"), False, False),
  "window": ("ffpa_attn_varlen_window_fwd", ("kv", "window"), False, False),
  "softcap": ("ffpa_attn_varlen_softcap_fwd", ("kv", "window"), True, False),
  "mla": ("ffpa_attn_varlen_mla_fwd", ("kv", "mla"), False, True),
  "mla_tree": ("ffpa_attn_varlen_mla_tree_fwd", ("kv", "mla", "tree"), False, True),
  "sparse": ("ffpa_attn_varlen_mla_sparse_fwd", ("sparse",), False, False),
  "mla_fp8": ("ffpa_attn_varlen_mla_fp8_fwd", ("kv", "mla", "fp8"), False, True),
  "mla_tree_fp8": ("ffpa_attn_varlen_mla_tree_fp8_fwd", ("kv", "mla", "tree", "fp8"), False, True),
  "sparse_fp8": ("ffpa_attn_varlen_mla_sparse_fp8_fwd", ("sparse", "fp8"), False, False),
  "sparse_ds": ("ffpa_attn_varlen_mla_sparse_ds_fwd", ("sparse",), False, False),
}
# the forms over the one latent cache (their kernels are named after the call alone) and, of those, the ones recorded later than the first eight forms: their
# entries stand behind the first eight's and are never folded into one of them, so that recording a new form leaves every older line of the list as it is
LATENT_FORMS = ("mla", "mla_tree", "sparse", "mla_fp8", "mla_tree_fp8", "sparse_fp8", "sparse_ds")
LATER_FORMS = ("mla_fp8", "mla_tree_fp8", "sparse_fp8", "sparse_ds")


def _hip():
  if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
  from ffpa_attn_amd import hip

  return hip


def _fill(struct, over: dict):
  for key, val in over.items():
    if isinstance(val, list):
      arr = getattr(struct, key)
      for i, x in enumerate(val):
        arr[i] = x
    else:
      setattr(struct, key, float(val) if isinstance(val, str) else val)
  return struct


def _structs(hip, call: dict):
  """The ctypes arguments of a call: params and the form's structs, each stamped with its size (and version) before the overrides."""
  classes = {"kv": hip.FfpaPagedKv, "tree": hip.FfpaTreeMask, "window": hip.FfpaWindow, "mla": hip.FfpaMla, "sparse": hip.FfpaMlaSparse,
             "fp8": hip.FfpaMlaFp8}
  keep, args = [], []
  for name, cls in [("params", hip.FfpaVarlenFwdParams)] + [(n, classes[n]) for n in FORMS[call["form"]][1]]:
    over = call.get(name, {})
    if over is None:
      args.append(None)
      continue
    s = _fill(hip._stamped(cls), full(call["form"], name, over))
    keep.append(s)
    args.append(ctypes.byref(s))
  if FORMS[call["form"]][2]:
    args.append(ctypes.c_float(float(call.get("softcap", SOFTCAP))))
  return keep, args


def replay(lib, call: dict, launch: bool = True) -> dict:
  """Run one call of the list through every export of its form and return what the library answered (the layout of ``got``)."""
  hip = _hip()
  stem, _, _, has_slots = FORMS[call["form"]]
  old = os.environ.pop("FFPA_HIP_FAKE_CUS", None)
  if call.get("cus") is not None:
    os.environ["FFPA_HIP_FAKE_CUS"] = str(call["cus"])
  try:
    keep, args = _structs(hip, call)
    null_out = bool(call.get("null_out"))
    err = lambda rc: lib.ffpa_attn_last_error().decode() if rc != 0 else ""
    got = {}
    plan = (ctypes.c_int * 5)(*([-7] * 5))
    rc = getattr(lib, stem + "_plan")(*args, None if null_out else plan)
    got["plan"] = [rc, err(rc), list(plan) if rc == 0 and not null_out else None]
    buf = ctypes.create_string_buffer(256)
    rc = getattr(lib, stem + "_kernel")(*args, None if null_out else buf, len(buf))
    got["kernel"] = [rc, err(rc), buf.value.decode() if rc == 0 and not null_out else None]
    got["workspace_bytes"] = int(getattr(lib, stem + "_workspace_bytes")(*args))
    if has_slots:
      slots = ctypes.c_int(-7)
      rc = getattr(lib, stem + "_compact_slots")(*args, None if null_out else ctypes.byref(slots))
      got["compact_slots"] = [rc, err(rc), slots.value if rc == 0 and not null_out else None]
    if launch:
      rc = getattr(lib, stem)(*args, None)
      got["launch"] = [rc, err(rc)]
    del keep
    return got
  finally:
    os.environ.pop("FFPA_HIP_FAKE_CUS", None)
    if old is not None:
      os.environ["FFPA_HIP_FAKE_CUS"] = old


QUERIES = ("plan", "kernel", "workspace_bytes", "compact_slots")


def kernel_stem(call: dict) -> "str | None":
  """What the kernels of the calls over a K and a V cache are named after — the cache, then the call — and the one thing in which those calls' answers to one
  set of arguments differ: the list writes it ``*``, so that they stay one entry."""
  if call["form"] in LATENT_FORMS:
    return None
  paged = call["form"] == "paged" or (call["form"] != "packed" and call.get("kv", {}) is not None)
  return "ffpa_fwd_m16_" + ("paged" if paged else "varlen") + {"packed": "", "paged": ""}.get(call["form"], "_" + call["form"]) + "_kernel"


def pack(got: dict, call: dict, base: "dict | None" = None) -> dict:
  """The short form of what ``replay`` returned (module docstring); ``base``: what the same call answered without its params overrides."""
  ok, refusal = got["plan"][0] == 0, got["plan"][:2]
  out = {"plan": got["plan"][2] if ok else refusal}
  for short, key in (("kernel", "kernel"), ("slots", "compact_slots")):
    if key in got and (got[key][0] == 0 or got[key][:2] != refusal):
      out[short] = got[key][2] if got[key][0] == 0 else got[key][:2]
  stem = kernel_stem(call)
  if stem and isinstance(out.get("kernel"), str) and out["kernel"].startswith(stem):
    out["kernel"] = "*" + out["kernel"][len(stem):]
  if got["workspace_bytes"]:
    out["ws"] = got["workspace_bytes"]
  if ok and got["launch"] != NO_DEVICE and base is not None and all(got.get(k) == base.get(k) for k in QUERIES):
    out = {"plan": "base"}  # (a call only the launch export refuses — a pointer, a stride, the scale —: its overrides change no query's answer)
  if got["launch"] != (NO_DEVICE if ok else refusal):
    out["launch"] = got["launch"]
  return out


def unpack(short: dict, call: dict, base: "dict | None" = None) -> dict:
  """The long form of a recorded ``got``: what ``replay`` returns for the call if the library answers as recorded."""
  form = call["form"]
  if isinstance(short.get("kernel"), str) and short["kernel"].startswith("*"):
    short = dict(short, kernel=kernel_stem(call) + short["kernel"][1:])
  if short["plan"] == "base":
    return dict({k: base[k] for k in QUERIES if k in base}, launch=list(short.get("launch", NO_DEVICE)))
  ok = not isinstance(short["plan"][1], str)
  refusal = None if ok else list(short["plan"])
  long_of = lambda v: list(refusal) + [None] if v is None else (list(v) + [None] if isinstance(v, list) else [0, "", v])
  got = {"plan": [0, "", list(short["plan"])] if ok else refusal + [None], "kernel": long_of(short.get("kernel")), "workspace_bytes": short.get("ws", 0)}
  if FORMS[form][3]:
    got["compact_slots"] = long_of(short.get("slots"))
  got["launch"] = list(short.get("launch", NO_DEVICE if ok else refusal))
  return got


def _base_key(call: dict) -> str:
  """What a call shares with its base: the form and every struct it passes but the params."""
  return json.dumps([call["form"], call.get("softcap")] + [call.get(n, {}) for n in FORMS[call["form"]][1]], sort_keys=True)


def _is_base(call: dict) -> bool:
  return call.get("params", {}) == {} and "cus" not in call and "null_out" not in call


def load(path: str = OUT) -> list:
  """``[(line of the file, call, the long form of what was recorded for it)]``: every call of the list, one per form of an entry."""
  with open(path) as f:
    entries = json.load(f)
  calls = [(line, dict(e, form=form)) for line, e in enumerate(entries, 2) for form in ([e["form"]] if isinstance(e["form"], str) else e["form"])]
  base = {_base_key(c): unpack(c["got"], c) for _, c in calls if _is_base(c)}
  return [(line, c, unpack(c["got"], c, base.get(_base_key(c)))) for line, c in calls]


# ------------------------------------------------------------------------------------ the list
Q, K, V, O, LSE, CU_Q, CU_K, USED, WS = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000, 0x6000, 0x6400, 0x6800, 0x7000
TABLE, BITS, KV_NEW, SEQLENS, INDICES, LENS = 0x8000, 0x8400, 0x9000, 0x8800, 0xA000, 0x8C00
BIG = 1 << 40
FORCE, STREAM, NO_STREAM, DET, NO_PACK, NO_COMPACT = 0x40, 0x80, 0x800, 0x4000, 0x40000, 0x400000


def params(hq=4, hkv=4, d=128, batch=2, mq=64, mkv=512, total_q=None, **over) -> dict:
  p = dict(q=Q, k=K, v=V, o=O, cu_seqlens_q=CU_Q, cu_seqlens_kv=CU_K, seqused_kv=USED, batch=batch, heads_q=hq, heads_kv=hkv, head_dim=d, max_seqlen_q=mq,
           max_seqlen_kv=mkv, q_stride=[hq * d, d], k_stride=[hkv * d, d], v_stride=[hkv * d, d], o_stride=[hq * d, d], softmax_scale=0.125,
           rescale_threshold=-1.0, total_q=batch * mq if total_q is None else total_q)
  p.update(over)
  return p


def scratch(**over) -> dict:
  return dict(workspace=WS, workspace_bytes=BIG, **over)


KV = dict(block_table=TABLE, bt_stride=64, pages_per_row=64, page_size=64, num_pages=4096, k_page_stride=64 * 4 * 128, v_page_stride=64 * 4 * 128)
TREE = dict(bits=BITS, batch_stride=0, tokens=64)
WINDOW = dict(left=100, right=0)
MLA = dict(head_dim_v=512)
SOFTCAP = 30.0
SPARSE = dict(indices=INDICES, indices_stride=256, topk_lens=LENS, kv_stride=[576, 576], topk=256, num_rows=100000, head_dim_v=512)

FP8 = dict(kv_scale=0.5)
SPARSE_DS = dict(SPARSE, kv_stride=[656, 656])  # (a pool of 656-byte rows: its strides are bytes)

STRIDES = {"q_stride": "heads_q", "k_stride": "heads_kv", "v_stride": "heads_kv", "o_stride": "heads_q"}  # a dense [T, H, D] layout: (H * D, D)


def latent_params(hq=16, d=576, **over) -> dict:
  over.setdefault("mq", 1)
  return params(hq=hq, hkv=1, d=d, **over)


def latent_kv() -> dict:
  return dict(KV, k_page_stride=64 * 576, v_page_stride=64 * 576)


def defaults(form: str, name: str) -> dict:
  """The fields of struct ``name`` that a call of ``form`` starts from (the params without their strides: ``full`` derives them)."""
  latent = form in LATENT_FORMS
  if name == "params":
    return {k: v for k, v in (latent_params() if latent else params()).items() if k not in STRIDES and k != "total_q"}
  return {"kv": latent_kv() if latent else KV, "tree": TREE, "window": WINDOW, "mla": MLA, "sparse": SPARSE_DS if form == "sparse_ds" else SPARSE, "fp8": FP8}[name]


def full(form: str, name: str, over: dict) -> dict:
  """Every field of the struct: the form's defaults, the call's overrides and — params — dense strides for the heads and the head dim it ends up with."""
  fields = dict(defaults(form, name), **over)
  if name == "params":
    for key, heads in STRIDES.items():
      fields.setdefault(key, [fields[heads] * fields["head_dim"], fields["head_dim"]])
    fields.setdefault("total_q", fields["batch"] * fields["max_seqlen_q"])  # (a uniform batch)
  return fields

CALLS: list[dict] = []


def _per_split(P: dict) -> int:
  """Scratch bytes of one KV range: fp32 partials of the kernel's head dim + one LSE per (query head, token)."""
  return P["heads_q"] * P["total_q"] * (max(128, (P["head_dim"] + 63) // 64 * 64) + 1) * 4


# What a regime's row must have reached when it is recorded, by its label: (the five plan integers, the kernel name, the call's params) -> bool.  The recorder
# refuses to write a list in which a row answers something else than its label says (a window that prices the splits away, a shape that no longer packs).
REACHED = {
  "plain rows": lambda p, k, P: p[0] == 1 and p[4] == 1 and "packed" not in k and "NT" not in k,
  "gqa rows packed": lambda p, k, P: "(GQA heads packed into rows)" in k,
  "gqa rows not packed by flag": lambda p, k, P: "packed" not in k,
  "several row tiles": lambda p, k, P: p[0] > 1,
  "compact grid": lambda p, k, P: p[3] < P["batch"] * P["heads_q"] * p[0],
  "nt by rule": lambda p, k, P: ", NT>" in k,
  "nt forced on": lambda p, k, P: ", NT>" in k,
  "nt forced off": lambda p, k, P: "NT" not in k,
  "splits by fill": lambda p, k, P: p[4] > 5 and "merge" in k,  # (more than either cap below leaves)
  "splits by fill 64 cus": lambda p, k, P: p[4] == 32,  # (128 slots over 4 workgroups, or 64 over 2: the device's size decides, not the tiles)
  "splits by fill 8 cus": lambda p, k, P: p[4] == 4,     # (the sparse call's 2048 rows are 64 tiles: a smaller device still)
  "splits by balance": lambda p, k, P: p[4] > 1,
  "splits forced": lambda p, k, P: p[4] == P["num_splits"],
  "splits capped by num_splits": lambda p, k, P: p[4] == P["num_splits"],
  "splits capped by workspace_bytes": lambda p, k, P: p[4] == P["workspace_bytes"] // _per_split(P) > 1,
  "deterministic": lambda p, k, P: p[4] == 1,
  "head dim below the first build": lambda p, k, P: ", 128" in k,
  "fp16": lambda p, k, P: "<fp16" in k,
  "heads packed": lambda p, k, P: "(heads packed into rows)" in k,
  "heads packed chunked": lambda p, k, P: "(heads packed into rows, chunked)" in k,
  "heads not packed by flag": lambda p, k, P: "packed" not in k,
  "compact grid unpacked": lambda p, k, P: "packed" not in k and "(compact grid)" in k,
  "compact grid packed": lambda p, k, P: "chunked" in k and "(compact grid)" in k,
}


def two_cache_regimes() -> list:
  """(label, params overrides, cus) of one accepted call per plan regime of the calls over a K and a V cache (D = 128: 128-row tiles)."""
  fill = dict(batch=2, hq=8, hkv=2, mq=1, mkv=16384, **scratch())
  return [
    ("plain rows", {}, None),
    ("gqa rows packed", dict(hq=8, hkv=2, mq=4), None),
    ("gqa rows not packed by flag", dict(hq=8, hkv=2, mq=4, flags=NO_PACK), None),
    ("several row tiles", dict(mq=1000), None),
    ("compact grid", dict(batch=16, mq=4096, mkv=4096, total_q=4336), None),
    ("nt by rule", dict(batch=64, hq=8, hkv=8, mq=1, mkv=8192), None),
    ("nt forced on", dict(flags=STREAM), None),
    ("nt forced off", dict(batch=64, hq=8, hkv=8, mq=1, mkv=8192, flags=NO_STREAM), None),
    ("splits by fill", fill, None),
    ("splits by fill 64 cus", fill, 64),
    ("splits by balance", dict(batch=32, hq=32, hkv=8, mq=1, mkv=16384, **scratch()), None),
    ("splits forced", dict(mq=1000, mkv=4096, num_splits=3, flags=FORCE, **scratch()), None),
    ("splits capped by num_splits", dict(fill, num_splits=5), None),
    ("splits capped by workspace_bytes", dict(fill, workspace_bytes=3 * 8 * 2 * 129 * 4 + 7), None),
    ("deterministic", dict(fill, flags=DET), None),
    ("head dim below the first build", dict(d=64), None),
    ("fp16", dict(dtype=1, hq=8, hkv=2, mq=4), None),
  ]


def latent_regimes() -> list:
  """... of the calls over the one latent cache (D = 576, dv = 512: 64-row tiles; one latent head)."""
  fill = dict(batch=2, hq=16, mq=1, mkv=16384, **scratch())
  return [
    ("heads packed", dict(hq=16, mq=1), None),
    ("heads packed chunked", dict(hq=128, mq=2), None),
    ("heads not packed by flag", dict(hq=16, mq=4, flags=NO_PACK), None),
    ("compact grid unpacked", dict(hq=1, batch=16, mq=2048, mkv=2048, total_q=2048 + 15), None),
    ("compact grid packed", dict(hq=128, batch=6, mq=40, mkv=4096, total_q=45), None),
    ("nt by rule", dict(batch=64, hq=16, mq=1, mkv=8192), None),
    ("nt forced on", dict(hq=16, mq=1, flags=STREAM), None),
    ("nt forced off", dict(batch=64, hq=16, mq=1, mkv=8192, flags=NO_STREAM), None),
    ("splits by fill", fill, None),
    ("splits by fill 64 cus", fill, 64),
    ("splits by balance", dict(batch=200, hq=16, mq=1, mkv=16384, **scratch()), None),
    ("splits forced", dict(hq=16, mq=1, mkv=4096, num_splits=3, flags=FORCE, **scratch()), None),
    ("splits capped by num_splits", dict(fill, num_splits=5), None),
    ("splits capped by workspace_bytes", dict(fill, workspace_bytes=3 * 16 * 2 * 577 * 4 + 7), None),
    ("deterministic", dict(fill, flags=DET), None),
    ("fp16", dict(dtype=1, hq=16, mq=1), None),
  ]


def common_refusals() -> list:
  """(label, params overrides | None) the packed call's plan and the launch's common checks refuse, in their order."""
  return [
    ("params NULL", None),
    ("params size", dict(struct_size=8)),
    ("dtype", dict(dtype=2)),
    ("batch zero", dict(batch=0)),
    ("heads not a multiple", dict(heads_q=5, heads_kv=2)),
    ("head dim not a multiple of 8", dict(head_dim=100)),
    ("grid too large", dict(batch=1 << 20, heads_q=1 << 12, heads_kv=1 << 12, max_seqlen_q=1)),
    ("q NULL", dict(q=0)),
    ("v NULL", dict(v=0)),
    ("cu_seqlens_q NULL", dict(cu_seqlens_q=0)),
    ("cu_seqlens_kv NULL", dict(cu_seqlens_kv=0)),
    ("cu_seqlens_kv misaligned", dict(cu_seqlens_kv=CU_K + 2)),
    ("seqused_kv misaligned", dict(seqused_kv=USED + 1)),
    ("q misaligned", dict(q=Q + 8)),
    ("q stride negative", dict(q_stride=[-128, 128])),
    ("k stride not 16 bytes", dict(k_stride=[1028, 128])),
    ("k rows overlap", dict(k_stride=[64, 128])),
    ("lse stride negative", dict(lse=LSE, lse_stride_head=-1)),
    ("scale not finite", dict(softmax_scale="nan")),
    ("total_q negative", dict(total_q=-1)),
    ("workspace misaligned", dict(workspace=WS + 4, workspace_bytes=BIG)),
    # two at once: which comes first
    ("q NULL and scale", dict(q=0, softmax_scale="nan")),
    ("head dim and o misaligned", dict(head_dim=4, o=O + 2)),
  ]


def add(form: str, label: str, p, cus=None, null_out=False, reached=None, **structs):
  def over(name, fields):  # (the fewest overrides from which full() restores the fields)
    if fields is None:
      return None
    base = defaults(form, name)
    derived = tuple(STRIDES) + ("total_q",) if name == "params" else ()
    out = {k: v for k, v in fields.items() if k not in derived and (k not in base or base[k] != v)}
    out.update({k: v for k, v in fields.items() if k in derived and v != full(form, name, out)[k]})
    assert full(form, name, out) == dict(base, **fields), (form, label, name)
    return out

  call = {"name": f"{form}: {label}", "form": form, "params": over("params", p)}
  if reached is not None:
    call["reached"] = lambda plan, kernel: reached(plan, kernel, p)
  if cus is not None:
    call["cus"] = cus
  if null_out:
    call["null_out"] = True
  for name in FORMS[form][1]:
    call[name] = over(name, structs[name])
  if FORMS[form][2] and structs["softcap"] != SOFTCAP:
    call["softcap"] = structs["softcap"]
  CALLS.append(call)


def build_list():
  # ---- the calls over a K and a V cache: packed, paged, tree x 2 caches, window x 2 caches, softcap with / without a window x 2 caches
  shapes = [
    ("packed", "", dict()),
    ("paged", "", dict(kv=KV)),
    ("tree", " (contiguous)", dict(kv=None, tree=TREE)),
    ("tree", " (paged)", dict(kv=KV, tree=TREE)),
    ("window", " (contiguous)", dict(kv=None, window=WINDOW)),
    ("window", " (paged)", dict(kv=KV, window=WINDOW)),
    ("softcap", " (contiguous, no window)", dict(kv=None, window=None, softcap=30.0)),
    ("softcap", " (paged, window)", dict(kv=KV, window=WINDOW, softcap=30.0)),
  ]
  # (a window of 100 keys prices the KV ranges away: the rows that are about the split count or the NT rule run under one that reaches past max_seqlen_kv — no left bound, causal)
  wide = dict(left=20000, right=0)
  for form, tag, structs in shapes:
    tree = "tree" in structs
    for label, over, cus in two_cache_regimes():
      if tree and label == "splits forced":
        over = dict(over, mq=16)  # (a tree holds at most 64 tokens: one row tile)
      if tree and over.get("mq", 64) > 64:
        continue  # (... so it has no regime of several row tiles)
      about_splits = label.startswith(("splits", "nt ")) or label == "deterministic"  # (the NT rule reads the priced length too)
      add(form, label + tag, params(**over), cus, reached=REACHED[label], **dict(structs, window=wide) if about_splits and structs.get("window") else structs)
    base = params()
    for label, over in common_refusals():
      add(form, "common: " + label + tag, None if over is None else dict(base, **over), **structs)
    add(form, "NULL out / buf" + tag, base, null_out=True, **structs)
    add(form, "refused: params size, NULL out" + tag, dict(base, struct_size=4), null_out=True, **structs)

  # ---- the window call: a left bound that lowers the priced max_seqlen_kv, and ones that do not
  for kv in (None, KV):
    tag = " (paged)" if kv else " (contiguous)"
    long_ctx = dict(batch=64, hq=8, hkv=8, mq=1, mkv=65536, **scratch())
    for label, w in [("left lowers the priced length", dict(left=1000, right=0)), ("left past the cache", dict(left=70000, right=-1)),
                     ("left lowers nothing", dict(left=65500, right=0)), ("unbounded", dict(left=-1, right=-1)), ("right only", dict(left=-1, right=3)),
                     ("left only", dict(left=4096, right=-1)), ("right past the tokens", dict(left=10, right=500))]:
      add("window", label + tag, params(**long_ctx), kv=kv, window=w)
      if label in ("left lowers the priced length", "left lowers nothing"):
        add("softcap", label + tag, params(**long_ctx), kv=kv, window=w, softcap=30.0)
    add("window", "left lowers the priced length, prefill rows" + tag, params(batch=1, hq=8, hkv=8, mq=1024, mkv=16384, causal=1, **scratch()), kv=kv, window=dict(left=512, right=-1))
    halved = params(batch=2, hq=8, hkv=2, mq=1, mkv=16384, num_splits=5, **scratch())
    add("window", "left halves the priced length, splits capped by num_splits" + tag, halved, kv=kv, window=dict(left=8192, right=-1), reached=REACHED["splits capped by num_splits"])
    add("softcap", "left halves the priced length, splits capped by num_splits" + tag, halved, kv=kv, window=dict(left=8192, right=-1), softcap=30.0,
        reached=REACHED["splits capped by num_splits"])
    add("window", "left lowers the priced length, packed rows" + tag, params(batch=4, hq=8, hkv=2, mq=8, mkv=16384, **scratch()), kv=kv, window=dict(left=300, right=2))
    # the window's own refusals
    for label, w in [("window NULL", None), ("window size", dict(struct_size=8)), ("window reserved", dict(reserved=1)), ("window left", dict(left=-2)),
                     ("window right", dict(right=-5)), ("window size and left", dict(struct_size=12, left=-9))]:
      add("window", "refused: " + label + tag, params(), kv=kv, window=None if w is None else dict(WINDOW, **w))
      if w is not None:
        add("softcap", "refused: " + label + tag, params(), kv=kv, window=dict(WINDOW, **w), softcap=30.0)
    add("window", "refused: window NULL and dtype" + tag, params(dtype=3), kv=kv, window=None)
    add("window", "refused: window left and q NULL" + tag, params(q=0), kv=kv, window=dict(left=-3, right=0))
    for label, cap in [("softcap zero", 0.0), ("softcap negative", -1.0), ("softcap nan", "nan"), ("softcap inf", "inf")]:
      add("softcap", "refused: " + label + tag, params(), kv=kv, window=WINDOW, softcap=cap)
    add("softcap", "refused: softcap and params NULL" + tag, None, kv=kv, window=WINDOW, softcap=0.0)
    add("softcap", "refused: softcap and window size" + tag, params(), kv=kv, window=dict(WINDOW, struct_size=4), softcap=-2.0)

  # ---- the page pool's refusals, for every call that takes one
  pool = [("kv size", dict(struct_size=40)), ("block_table NULL", dict(block_table=0)), ("block_table misaligned", dict(block_table=TABLE + 2)),
          ("page_size", dict(page_size=96)), ("pages_per_row", dict(pages_per_row=0)),
          ("keys per sequence", dict(pages_per_row=1 << 26, bt_stride=1 << 26)), ("bt_stride", dict(bt_stride=63)), ("k page stride negative", dict(k_page_stride=-8)),
          ("v page stride not 16 bytes", dict(v_page_stride=1028)), ("kv size and page_size", dict(struct_size=0, page_size=1))]
  takers = [("paged", dict(), params(), False), ("tree", dict(tree=TREE), params(), False), ("window", dict(window=WINDOW), params(), False),
            ("softcap", dict(window=None, softcap=30.0), params(), False), ("mla", dict(mla=MLA), latent_params(), True),
            ("mla_tree", dict(mla=MLA, tree=TREE), latent_params(), True)]
  for form, structs, base, latent in takers:
    for label, over in pool:
      add(form, "refused: " + label, base, kv=dict(latent_kv() if latent else KV, **over), **structs)
    add(form, "refused: seqused_kv NULL", dict(base, seqused_kv=0), kv=latent_kv() if latent else KV, **structs)
    add(form, "refused: seqused_kv NULL and page_size", dict(base, seqused_kv=0), kv=dict(KV, page_size=100), **structs)
    add(form, "refused: pool and k NULL", dict(base, k=0), kv=dict(KV, bt_stride=1), **structs)
    if form in ("paged", "mla", "mla_tree"):
      add(form, "refused: kv NULL", base, kv=None, **structs)
      add(form, "refused: kv NULL and params NULL", None, kv=None, **structs)
      add(form, "refused: kv NULL and dtype", dict(base, dtype=9), kv=None, **structs)

  # ---- the tree mask's refusals, for both calls that take one
  masks = [("tree NULL", None), ("tree size", dict(struct_size=16)), ("bits NULL", dict(bits=0)), ("bits misaligned", dict(bits=BITS + 4)), ("tokens zero", dict(tokens=0)),
           ("tokens above 64", dict(tokens=65)), ("max_seqlen_q above tokens", dict(tokens=8)), ("batch_stride", dict(batch_stride=5, tokens=64)),
           ("per-sequence masks", dict(batch_stride=64)), ("bits NULL and tokens", dict(bits=0, tokens=100))]
  for form, structs, base, kvs in [("tree", dict(), params(), (None, KV)), ("mla_tree", dict(mla=MLA), latent_params(), (latent_kv(),))]:
    for kv in kvs:
      tag = "" if form == "mla_tree" else (" (paged)" if kv else " (contiguous)")
      for label, over in masks:
        accepted = label == "per-sequence masks"
        add(form, ("" if accepted else "refused: ") + label + tag, dict(base, max_seqlen_q=16, total_q=32), kv=kv, tree=None if over is None else dict(TREE, **over), **structs)
      add(form, "refused: tree NULL and scale" + tag, dict(base, softmax_scale="inf"), kv=kv, tree=None, **structs)
      add(form, "refused: tokens and head dim" + tag, dict(base, head_dim=0), kv=kv, tree=dict(TREE, tokens=0), **structs)
      if kv is not None:
        add(form, "refused: tree size and pool" + tag, base, kv=dict(kv, num_pages=0), tree=dict(TREE, struct_size=1), **structs)

  # ---- the latent calls
  def latent_calls(form, structs):
    for label, over, cus in latent_regimes():
      if "tree" in structs and over.get("mq", 1) > 64:
        continue  # (a tree holds at most 64 tokens)
      add(form, label, latent_params(**over), cus, reached=REACHED[label], kv=latent_kv(), mla=MLA, **structs)
    add(form, "causal flag set by the caller", latent_params(hq=16, mq=8, causal=1), kv=latent_kv(), mla=MLA, **structs)
    add(form, "append in front", latent_params(hq=16, mq=2), kv=latent_kv(), mla=dict(MLA, seqlen_new=2, kv_new=KV_NEW, cache_seqlens=SEQLENS, kv_new_stride=[1152, 576, 576]), **structs)
    base = latent_params()
    for label, over in common_refusals():
      add(form, "common: " + label, None if over is None else dict(base, **over), kv=latent_kv(), mla=MLA, **structs)
    add(form, "NULL out / buf / slots", base, null_out=True, kv=latent_kv(), mla=MLA, **structs)
    app = dict(MLA, seqlen_new=2, kv_new=KV_NEW, cache_seqlens=SEQLENS, kv_new_stride=[1152, 576, 576])
    for label, m in [("mla NULL", None), ("mla size", dict(struct_size=24)), ("mla reserved", dict(reserved=3)), ("head_dim_v zero", dict(head_dim_v=0)),
                     ("head_dim_v not a multiple of 64", dict(head_dim_v=500)), ("head_dim_v above head_dim", dict(head_dim_v=640)),
                     ("pair not built", dict(head_dim_v=256)), ("seqlen_new negative", dict(seqlen_new=-1)), ("kv_new NULL", dict(app, kv_new=0)),
                     ("cache_seqlens NULL", dict(app, cache_seqlens=0)), ("kv_new misaligned", dict(app, kv_new=KV_NEW + 4)),
                     ("cache_seqlens misaligned", dict(app, cache_seqlens=SEQLENS + 1)), ("cache_seqlens is seqused_kv", dict(app, cache_seqlens=USED)),
                     ("kv_new stride negative", dict(app, kv_new_stride=[-8, 576, 576])), ("kv_new stride not 16 bytes", dict(app, kv_new_stride=[1152, 580, 576])),
                     ("mla size and reserved", dict(struct_size=0, reserved=1)), ("pair and seqlen_new", dict(head_dim_v=128, seqlen_new=-4))]:
      add(form, "refused: " + label, base, kv=latent_kv(), mla=None if m is None else dict(MLA, **m), **structs)
    add(form, "refused: head dim not a multiple of 64", latent_params(d=200), kv=latent_kv(), mla=MLA, **structs)
    add(form, "refused: head dim 512 not built", latent_params(d=512), kv=latent_kv(), mla=MLA, **structs)
    add(form, "refused: grid of new rows", latent_params(batch=1 << 16, hq=1, mq=1), kv=latent_kv(), mla=dict(app, seqlen_new=1 << 16), **structs)
    add(form, "refused: mla NULL and pool", base, kv=dict(latent_kv(), page_size=1), mla=None, **structs)
    add(form, "refused: mla reserved and o NULL", dict(base, o=0), kv=latent_kv(), mla=dict(MLA, reserved=1), **structs)
  for form, structs in [("mla", dict()), ("mla_tree", dict(tree=TREE))]:
    latent_calls(form, structs)
  add("mla_tree", "refused: mla NULL and tree NULL", latent_params(), kv=latent_kv(), mla=None, tree=None)
  add("mla_tree", "refused: pair not built and tokens", latent_params(), kv=latent_kv(), mla=dict(MLA, head_dim_v=64), tree=dict(TREE, tokens=0))
  add("mla_tree", "refused: params size and tree NULL", dict(latent_params(), struct_size=16), kv=latent_kv(), mla=MLA, tree=None)

  # ---- the sparse latent call: T one-token sequences
  def sp(**over):
    return latent_params(mq=1, **over)

  def sparse_calls(form, S, geometry, structs):
    fill = dict(batch=2, hq=16, **scratch())
    for label, over, s, cus in [
      ("heads packed", dict(hq=16), {}, None), ("heads packed chunked", dict(hq=128), {}, None), ("heads not packed by flag", dict(hq=16, flags=NO_PACK), {}, None),
      ("nt by rule", dict(hq=16, batch=4096), dict(topk=2048, indices_stride=2048), None), ("nt forced on", dict(hq=16, flags=STREAM), {}, None),
      ("nt forced off", dict(hq=16, batch=4096, flags=NO_STREAM), dict(topk=2048, indices_stride=2048), None),
      ("splits by fill", fill, dict(topk=2048, indices_stride=2048), None), ("splits by fill 8 cus", fill, dict(topk=2048, indices_stride=2048), 8),
      ("splits by balance", dict(batch=200, hq=2, **scratch()), dict(topk=2048, indices_stride=4096), None),  # (few heads: the partials stay cheap next to 2048 rows)
      ("splits forced", dict(hq=16, num_splits=3, flags=FORCE, **scratch()), {}, None),
      ("splits capped by num_splits", dict(fill, num_splits=2), dict(topk=2048, indices_stride=2048), None),
      ("splits capped by workspace_bytes", dict(fill, workspace_bytes=2 * 16 * 2 * 577 * 4 + 100), dict(topk=2048, indices_stride=2048), None),
      ("deterministic", dict(fill, flags=DET), dict(topk=2048, indices_stride=2048), None),
      ("causal flag set by the caller", dict(hq=16, causal=1), {}, None), ("topk_lens NULL", dict(hq=16), dict(topk_lens=0), None),
      ("fp16", dict(hq=16, dtype=1), {}, None),
    ]:
      if form == "sparse_ds" and label == "fp16":
        add(form, "refused: fp16", sp(**over), sparse=dict(S, **s))  # (the rows' rotary columns are bf16: the pool's geometry refuses any other q)
        continue
      add(form, label, sp(**over), cus, reached=REACHED.get(label), sparse=dict(S, **s), **structs)
    base = sp()
    for label, over in common_refusals():
      add(form, "common: " + label, None if over is None else dict(base, **over), sparse=S, **structs)
    add(form, "NULL out / buf", base, null_out=True, sparse=S, **structs)
    for label, s in [("sparse NULL", None), ("sparse size", dict(struct_size=48)), ("sparse reserved", dict(reserved=1)), ("sparse reserved2", dict(reserved2=1)),
                     ("topk zero", dict(topk=0)), ("num_rows zero", dict(num_rows=0)), ("indices NULL", dict(indices=0)), ("indices misaligned", dict(indices=INDICES + 2)),
                     ("topk_lens misaligned", dict(topk_lens=LENS + 1)), ("indices_stride", dict(indices_stride=255)), ("head_dim_v zero", dict(head_dim_v=0)),
                     ("pair not built", dict(head_dim_v=256))] + geometry + [
                     ("sparse size and topk", dict(struct_size=1, topk=-1)), ("indices and kv stride", dict(indices=0, kv_stride=[-1, 0]))]:
      add(form, "refused: " + label, base, sparse=None if s is None else dict(S, **s), **structs)
    add(form, "refused: max_seqlen_q above one", latent_params(mq=2), sparse=S, **structs)
    add(form, "refused: sparse NULL and params NULL", None, sparse=None, **structs)
    add(form, "refused: sparse size and params size", dict(base, struct_size=0), sparse=dict(S, struct_size=0), **structs)
    add(form, "refused: max_seqlen_q and dtype", dict(base, max_seqlen_q=3, dtype=5), sparse=S, **structs)
    add(form, "refused: topk and head dim", dict(base, head_dim=1), sparse=dict(S, topk=0), **structs)
    add(form, "refused: pool span and q misaligned", dict(base, q=Q + 2), sparse=dict(S, num_rows=1 << 30), **structs)

  # (the pool's geometry, counted in the pool's elements: 16-bit ones, bytes of an e4m3 pool — the same reach holds twice the rows —, bytes of 656-byte rows)
  geometry = [("kv stride negative", dict(kv_stride=[576, -8])), ("kv stride not 16 bytes", dict(kv_stride=[580, 576])),
              ("kv rows overlap", dict(kv_stride=[512, 576])), ("kv rows too far apart", dict(kv_stride=[1 << 24, 576]))]
  sparse_calls("sparse", SPARSE, geometry + [("pool span", dict(num_rows=2000000))], dict())

  # ---- the latent calls over pools counted in bytes (LATER_FORMS).  Every latent call applies the steps that its traits switch on, in ONE order:
  #   1 ffpa_mla_fp8 (e4m3)  2 ffpa_mla_sparse in front of the plan (gather)  3 the causal copy (tree)  4 the plan  5 the page pool (page table)  6 ffpa_mla
  #   7 the mask (tree)  8 the gathered pool's geometry (gather)  9 the e4m3 pool's strides (e4m3)
  # Each form gets one refusal per step it has and, for every two steps that follow each other in it, one call that breaks both: the earlier step answers.
  fp8s = [("fp8 NULL", None), ("fp8 size", dict(struct_size=8)), ("fp8 reserved", dict(reserved=1)), ("fp8 reserved2", dict(reserved2=1.0)),
          ("kv_scale zero", dict(kv_scale=0.0)), ("kv_scale negative", dict(kv_scale=-1.0)), ("kv_scale nan", dict(kv_scale="nan")), ("kv_scale inf", dict(kv_scale="inf")),
          ("fp8 size and kv_scale", dict(struct_size=0, kv_scale=0.0))]
  odd_page = dict(latent_kv(), k_page_stride=64 * 576 + 8, v_page_stride=64 * 576 + 8)  # (16 bytes of a 16-bit pool, not 16 elements of an e4m3 one)
  for form, structs in [("mla_fp8", dict(fp8=FP8)), ("mla_tree_fp8", dict(tree=TREE, fp8=FP8))]:
    tree = "tree" in structs
    rest = dict(structs, kv=latent_kv(), mla=MLA)
    base = latent_params()
    latent_calls(form, structs)  # (the plan — step 4 — through the common refusals, ffpa_mla — step 6 —, "mla NULL and pool": 5 + 6)
    add(form, "power-of-two scale above one", base, **dict(rest, fp8=dict(kv_scale=4.0)))
    for label, f in fp8s:  # step 1
      add(form, "refused: " + label, base, **dict(rest, fp8=None if f is None else dict(FP8, **f)))
    add(form, "refused: fp8 NULL and params NULL", None, **dict(rest, fp8=None))  # 1 + 3 / 4
    add(form, "refused: kv_scale and dtype", dict(base, dtype=2), **dict(rest, fp8=dict(kv_scale=0.0)))  # 1 + 4
    add(form, "refused: fp8 reserved and params size", dict(base, struct_size=16), **dict(rest, fp8=dict(FP8, reserved=7)))  # 1 + 3
    for label, over in pool:  # step 5
      add(form, "refused: " + label, base, **dict(rest, kv=dict(latent_kv(), **over)))
    add(form, "refused: seqused_kv NULL", dict(base, seqused_kv=0), **rest)
    add(form, "refused: kv NULL", base, **dict(rest, kv=None))
    add(form, "refused: kv NULL and dtype", dict(base, dtype=9), **dict(rest, kv=None))  # 4 + 5
    add(form, "refused: batch and page_size", dict(base, batch=0), **dict(rest, kv=dict(latent_kv(), page_size=96)))  # 4 + 5
    # step 9, alone and behind the step in front of it
    add(form, "refused: row stride not 16 elements", dict(base, k_stride=[584, 576]), **rest)
    add(form, "refused: head stride not 16 elements", dict(base, k_stride=[576, 584]), **rest)
    add(form, "refused: page stride not 16 elements", base, **dict(rest, kv=odd_page))
    add(form, "refused: row stride and o NULL", dict(base, k_stride=[584, 576], o=0), **rest)  # (9 + the launch's own checks)
    if tree:
      for label, over in masks:  # step 7
        accepted = label == "per-sequence masks"
        add(form, ("" if accepted else "refused: ") + label, dict(base, max_seqlen_q=16, total_q=32), **dict(rest, tree=None if over is None else dict(TREE, **over)))
      add(form, "not causal by the caller, several tokens", latent_params(hq=16, mq=8, causal=0), **rest)  # step 3: planned as the causal call is
      add(form, "refused: params size and tree NULL", dict(base, struct_size=16), **dict(rest, tree=None))  # 3 / 4 + 7
      add(form, "refused: pair not built and tokens", base, **dict(rest, mla=dict(MLA, head_dim_v=64), tree=dict(TREE, tokens=0)))  # 6 + 7
      add(form, "refused: mla NULL and tree NULL", base, **dict(rest, mla=None, tree=None))  # 6 + 7
      add(form, "refused: tree NULL and page stride", base, **dict(rest, kv=odd_page, tree=None))  # 7 + 9
      add(form, "refused: tokens and row stride", dict(base, k_stride=[584, 576]), **dict(rest, tree=dict(TREE, tokens=65)))  # 7 + 9
    else:
      add(form, "refused: mla reserved and page stride", base, **dict(rest, kv=odd_page, mla=dict(MLA, reserved=1)))  # 6 + 9
      add(form, "refused: pair not built and row stride", dict(base, k_stride=[584, 576]), **dict(rest, mla=dict(MLA, head_dim_v=256)))  # 6 + 9

  # the gather over an e4m3 pool: strides and span in bytes, one per element
  sparse_calls("sparse_fp8", SPARSE, geometry + [("pool span", dict(num_rows=4000000))], dict(fp8=FP8))  # (steps 2, 4, 6, 8; "max_seqlen_q and dtype": 2 + 4)
  base = sp()
  for label, f in fp8s:  # step 1
    add("sparse_fp8", "refused: " + label, base, sparse=SPARSE, fp8=None if f is None else dict(FP8, **f))
  add("sparse_fp8", "power-of-two scale above one", base, sparse=SPARSE, fp8=dict(kv_scale=4.0))
  add("sparse_fp8", "twice the rows of the 16-bit pool's reach", base, sparse=dict(SPARSE, num_rows=3000000), fp8=FP8)
  add("sparse_fp8", "refused: fp8 NULL and sparse NULL", base, sparse=None, fp8=None)  # 1 + 2
  add("sparse_fp8", "refused: kv_scale and topk", base, sparse=dict(SPARSE, topk=0), fp8=dict(kv_scale="nan"))  # 1 + 2
  add("sparse_fp8", "refused: fp8 NULL and params NULL", None, sparse=SPARSE, fp8=None)  # 1 + 2
  add("sparse_fp8", "refused: indices_stride and batch", dict(base, batch=0), sparse=dict(SPARSE, indices_stride=8), fp8=FP8)  # 2 + 4
  add("sparse_fp8", "refused: dtype and pair not built", dict(base, dtype=2), sparse=dict(SPARSE, head_dim_v=256), fp8=FP8)  # 4 + 6
  add("sparse_fp8", "refused: pair not built and kv stride", base, sparse=dict(SPARSE, head_dim_v=256, kv_stride=[576, -16]), fp8=FP8)  # 6 + 8
  add("sparse_fp8", "refused: head_dim_v and pool span", base, sparse=dict(SPARSE, head_dim_v=0, num_rows=1 << 30), fp8=FP8)  # 6 + 8
  add("sparse_fp8", "refused: row stride not 16 elements", base, sparse=dict(SPARSE, kv_stride=[584, 576]), fp8=FP8)  # step 9
  add("sparse_fp8", "refused: head stride not 16 elements", base, sparse=dict(SPARSE, kv_stride=[576, 8]), fp8=FP8)
  add("sparse_fp8", "refused: pool span and row stride", base, sparse=dict(SPARSE, kv_stride=[584, 576], num_rows=1 << 30), fp8=FP8)  # 8 + 9
  add("sparse_fp8", "refused: rows overlap and head stride", base, sparse=dict(SPARSE, kv_stride=[520, 8]), fp8=FP8)  # 8 + 9
  add("sparse_fp8", "refused: row stride and q NULL", dict(base, q=0), sparse=dict(SPARSE, kv_stride=[584, 576]), fp8=FP8)  # (9 + the launch's own checks)

  # the gather over 656-byte rows: strides and span in bytes, bf16 only, the one (576, 512) row format
  ds_geometry = [("kv stride negative", dict(kv_stride=[656, -16])), ("slot stride not 16 bytes", dict(kv_stride=[664, 656])), ("head stride not 16 bytes", dict(kv_stride=[656, 8])),
                 ("slots overlap", dict(kv_stride=[640, 656])), ("slots too far apart", dict(kv_stride=[1 << 24, 656])), ("pool span", dict(num_rows=4000000))]
  sparse_calls("sparse_ds", SPARSE_DS, ds_geometry, dict())  # (steps 2, 4, 6, 8; "max_seqlen_q and dtype": 2 + 4; its fp16 row: refused by step 8)
  add("sparse_ds", "padded slots", base, sparse=dict(SPARSE_DS, kv_stride=[704, 704]))
  add("sparse_ds", "refused: pool misaligned", dict(base, k=K + 8), sparse=SPARSE_DS)  # step 8
  add("sparse_ds", "refused: fp16 and slot stride", dict(base, dtype=1), sparse=dict(SPARSE_DS, kv_stride=[600, 656]))  # (inside step 8: the dtype first)
  add("sparse_ds", "refused: slot stride and pool misaligned", dict(base, k=K + 8), sparse=dict(SPARSE_DS, kv_stride=[600, 656]))
  add("sparse_ds", "refused: indices NULL and heads", dict(base, heads_q=5, heads_kv=2), sparse=dict(SPARSE_DS, indices=0))  # 2 + 4
  add("sparse_ds", "refused: dtype and pair not built", dict(base, dtype=2), sparse=dict(SPARSE_DS, head_dim_v=256))  # 4 + 6
  add("sparse_ds", "refused: pair not built and slot stride", base, sparse=dict(SPARSE_DS, head_dim_v=256, kv_stride=[600, 656]))  # 6 + 8
  add("sparse_ds", "refused: head_dim_v and fp16", dict(base, dtype=1), sparse=dict(SPARSE_DS, head_dim_v=0))  # 6 + 8


def main(argv):
  hip = _hip()
  path = argv[argv.index("--library") + 1] if "--library" in argv else None
  import torch

  assert not torch.cuda.is_available(), "record on a box without a GPU: an accepted call's launch export would launch on made-up addresses"
  lib = hip.load_library(path)
  build_list()
  names = [c["name"] for c in CALLS]
  assert len(names) == len(set(names)), sorted(n for n in names if names.count(n) > 1)
  accepted, answers, base = 0, [replay(lib, call) for call in CALLS], {}
  for call, got in zip(CALLS, answers):
    if _is_base(call):
      base[_base_key(call)] = got
  for call, got in zip(CALLS, answers):
    accepted += got["plan"][0] == 0
    reached = call.pop("reached", None)
    assert reached is None or (got["plan"][0] == 0 and reached(got["plan"][2], got["kernel"][2])), (call["name"], got["plan"], got["kernel"])
    if call["form"] in ("packed", "paged", "tree") and got["plan"][0] != 0 and not call.get("null_out"):
      # the one answer the list does not pin: these three sized a launch from the params alone, whatever their plan said of the pool or the mask — the contract
      # is 0 for arguments the call's plan refuses, as the other forms have always answered
      got["workspace_bytes"] = 0
    mine = None if _is_base(call) else base.get(_base_key(call))
    call["got"] = pack(got, call, mine)
    assert unpack(call["got"], call, mine) == got, call["name"]
    del call["name"]  # (the labels stay in this file: the list is identified by what it passes)
    for name in ("params",) + FORMS[call["form"]][1]:
      if call[name] == {}:
        del call[name]
  # calls that pass the same and were answered the same by several forms are one entry with the list of those forms ("kv": null means nothing to a form without a pool)
  merged = {}
  for call in CALLS:
    form = call.pop("form")
    if form == "packed":
      call["kv"] = None
    merged.setdefault(json.dumps(call, sort_keys=True) + str(form in LATER_FORMS), (call, []))[1].append(form)
  entries = [dict({"form": forms[0] if len(forms) == 1 else forms}, **call) for call, forms in merged.values()]
  with open(OUT, "w") as f:
    f.write("[\n" + ",\n".join(json.dumps(c, separators=(",", ":")) for c in entries) + "\n]\n")
  print(f"{OUT}: {len(entries)} entries, {len(CALLS)} calls ({accepted} accepted by *_plan), {os.path.getsize(OUT)} bytes, library {path or hip.LIB_PATH}")


if __name__ == "__main__":
  main(sys.argv[1:])
