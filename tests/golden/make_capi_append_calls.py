"""Record tests/golden/capi_append_calls.json: what the two KV-cache append exports of the C-ABI — ffpa_attn_kvcache_append and ffpa_attn_kvcache_append_varlen —
answer, call by call, WITHOUT a device.

    python tests/golden/make_capi_append_calls.py [--library PATH]

Run on a box without a GPU against the library whose behaviour is to be pinned (a host-layer refactor records it from the commit BEFORE the refactor and replays
it afterwards: tests/test_capi_append_calls.py).  Without a device a launch export that has passed every argument check answers NO_DEVICE, so the whole order of
the checks shows here; no tensor is read, so every pointer is a made-up, suitably aligned address (the conventions of make_capi_varlen_calls.py).

The file is a list of calls, one per line: ``at`` (where the call is made: "u" | "r" — the uniform or the ragged export — then "p" | "c" — a ``ffpa_paged_kv`` is
passed, or NULL and ``capacity`` counts; a call made alike and answered alike at several places stands once), ``params`` / ``kv`` (field overrides over
``DEFAULTS``: a valid call with k / v and the rotary tables; ``params`` null: the params pointer is NULL), ``why`` (the check or the two neighbouring checks the
call breaks — the earlier one answers — or what an accepted call varies) and ``got`` = ``[status, ffpa_attn_last_error()]``.  ``load()`` returns the calls one
by one, each as ``calls()`` lists it: ``export`` ("uniform" | "ragged"), ``paged``, ``why``, ``params``, ``kv``, ``got``."""

from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "capi_append_calls.json")
ERR_NO_DEVICE = 9
NO_DEVICE = [ERR_NO_DEVICE, "no current HIP device"]  # what a launch export answers on a box without a device once every argument check has passed

B, SQ, HQ, HKV, D, CAP, PAGE, PER_ROW, PAGES, RD = 2, 3, 4, 2, 64, 128, 64, 2, 4, 32
T = B * SQ
Q, K, V, KC, VC, QR, USED, LENS, COS, SIN, CU, POS, TABLE = (0x10000 * i for i in range(1, 14))
_COMMON = dict(q=Q, k=K, v=V, k_cache=KC, v_cache=VC, q_rot=QR, seqused=USED, cache_seqlens=LENS, rotary_cos=COS, rotary_sin=SIN, batch=B, heads_q=HQ, heads_kv=HKV,
               head_dim=D, capacity=CAP, seqlen_ro=CAP, rotary_dim=RD, rotary_interleaved=1, causal=0, dtype=0, k_cache_stride=[CAP * HKV * D, HKV * D, D],
               v_cache_stride=[CAP * HKV * D, HKV * D, D])
DEFAULTS = {
  "uniform": dict(_COMMON, seqlen_q=SQ, seqlen_new=SQ, q_stride=[SQ * HQ * D, HQ * D, D], q_rot_stride=[SQ * HQ * D, HQ * D, D], k_stride=[SQ * HKV * D, HKV * D, D],
                  v_stride=[SQ * HKV * D, HKV * D, D]),
  "ragged": dict(_COMMON, cu_seqlens_q=CU, total_q=T, q_stride=[HQ * D, D], q_rot_stride=[HQ * D, D], k_stride=[HKV * D, D], v_stride=[HKV * D, D]),
  "kv": dict(block_table=TABLE, bt_stride=PER_ROW, pages_per_row=PER_ROW, page_size=PAGE, num_pages=PAGES, k_page_stride=PAGE * HKV * D, v_page_stride=PAGE * HKV * D),
}
EXPORTS = {"uniform": ("ffpa_attn_kvcache_append", "FfpaKvAppendParams"), "ragged": ("ffpa_attn_kvcache_append_varlen", "FfpaKvAppendVarlenParams")}
_NO_ROTARY = dict(rotary_dim=0, seqlen_ro=0, q=0, q_rot=0, rotary_cos=0, rotary_sin=0)


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
      setattr(struct, key, val)
  return struct


def replay(lib, call: dict) -> list:
  """Run one call of the list and return ``[status, ffpa_attn_last_error()]`` (the layout of ``got``)."""
  hip = _hip()
  export, cls = EXPORTS[call["export"]]
  p = None if call.get("params", {}) is None else _fill(hip._stamped(getattr(hip, cls)), {**DEFAULTS[call["export"]], **call.get("params", {})})
  kv = _fill(hip._stamped(hip.FfpaPagedKv), {**DEFAULTS["kv"], **call.get("kv", {})}) if call["paged"] else None
  rc = getattr(lib, export)(ctypes.byref(p) if p is not None else None, ctypes.byref(kv) if kv is not None else None, None)
  return [rc, lib.ffpa_attn_last_error().decode() if rc != 0 else ""]


# ----------------------------------------------------------------------------------------------------------------------------- the calls
def check_order(export: str, paged: bool) -> "list[tuple[str, dict, dict]]":
  """One fault per check of the export, (why, params overrides, kv overrides), in the order the recorded library makes the checks."""
  u = export == "uniform"
  rows = "seqlen_new" if u else "total_q"
  chain = [("struct_size", dict(struct_size=8), {}), ("abi_version", dict(abi_version=1), {}), ("dtype", dict(dtype=2), {}), ("batch", dict(batch=0), {}),
           ("heads", dict(heads_q=3), {}), ("head_dim", dict(head_dim=12), {}), (rows + " negative", {rows: -1}, {})]
  chain += [("pool", {}, dict(page_size=32))] if paged else [("capacity", dict(capacity=0), {})]
  chain += [("rotary_dim", dict(rotary_dim=8), {}), ("seqlen_ro", dict(seqlen_ro=64), {}), ("caches NULL", dict(v_cache=0), {}), ("k / v NULL", dict(k=0), {}),
            ("tables NULL", dict(rotary_sin=0), {}), ("q / q_rot NULL", dict(q_rot=0), {})]
  chain += [] if u else [("positions without rotary", dict(positions=POS, **_NO_ROTARY), {})]
  chain += [("seqused is cache_seqlens", dict(seqused=LENS), {}), ("4-byte alignment", dict(cache_seqlens=LENS + 2), {}), ("16-byte alignment", dict(k_cache=KC + 8), {}),
            ("cache strides", dict(v_cache_stride=[CAP * HKV * D, HKV * D, 4]), {}), ("k / v strides", dict(k_stride=[-8] * (3 if u else 2)), {}),
            ("q / q_rot strides", dict(q_rot_stride=[12] * (3 if u else 2)), {})]
  chain += [("grid", dict(batch=70000, seqlen_new=40000), {})] if u else []
  return chain


def more_faults(export: str, paged: bool) -> "list[tuple[str, dict, dict]]":
  """The other ways of breaking a check that has several, the checks of the pool one by one, and the pairs a merge of two neighbours' overrides does not make."""
  u = export == "uniform"
  out = [("params NULL", None, {}), ("heads_kv", dict(heads_kv=0), {}), ("head_dim 1032", dict(head_dim=1032, rotary_dim=0), {}), ("rotary_dim negative", dict(rotary_dim=-16), {}),
         ("rotary_dim past head_dim", dict(rotary_dim=80), {}), ("k_cache NULL", dict(k_cache=0), {}), ("seqused NULL", dict(seqused=0), {}), ("v NULL", dict(v=0), {}),
         ("rotary_cos NULL", dict(rotary_cos=0), {}), ("q NULL", dict(q=0), {}), ("seqused misaligned", dict(seqused=USED + 1), {}), ("v misaligned", dict(v=V + 4), {}),
         ("q misaligned", dict(q=Q + 2), {}), ("rotary_cos misaligned", dict(rotary_cos=COS + 8), {}), ("k_cache stride negative", dict(k_cache_stride=[-8, 128, 64]), {}),
         ("v stride odd", dict(v_stride=[4] * (3 if u else 2)), {}), ("q stride odd", dict(q_stride=[4] * (3 if u else 2)), {}),
         ("seqused is cache_seqlens, both misaligned", dict(seqused=LENS + 2, cache_seqlens=LENS + 2), {}),
         ("16-byte alignment + cache strides", dict(k_cache=KC + 8, k_cache_stride=[8, 8, 4]), {})]
  if u:
    out += [("seqlen_q negative", dict(seqlen_q=-1), {})]
  else:
    out += [("cu_seqlens_q NULL", dict(cu_seqlens_q=0), {}), ("cu_seqlens_q misaligned", dict(cu_seqlens_q=CU + 2), {}), ("positions misaligned", dict(positions=POS + 2), {}),
            ("positions without rotary + seqused is cache_seqlens", dict(positions=POS, seqused=LENS, **_NO_ROTARY), {})]
  if paged:
    out += [("pool: struct_size", {}, dict(struct_size=8)), ("pool: block_table NULL", {}, dict(block_table=0)), ("pool: block_table misaligned", {}, dict(block_table=TABLE + 2)),
            ("pool: page_size 0", {}, dict(page_size=0)), ("pool: pages_per_row", {}, dict(pages_per_row=0)), ("pool: num_pages", {}, dict(num_pages=0)),
            ("pool: keys per sequence", {}, dict(pages_per_row=1 << 26, bt_stride=1 << 26)), ("pool: bt_stride", {}, dict(bt_stride=1)),
            ("pool: page stride negative", {}, dict(k_page_stride=-8)), ("pool: page stride odd", {}, dict(v_page_stride=4)),
            ("seqlen_ro against the pool's capacity", dict(seqlen_ro=CAP), dict(pages_per_row=3, bt_stride=3))]
  else:
    out += [("capacity negative", dict(capacity=-64), {})]
  return out


def accepted(export: str) -> "list[tuple[str, dict, dict]]":
  u = export == "uniform"
  no_rows = dict(seqlen_new=0, k=0, v=0) if u else dict(total_q=0, k=0, v=0, q=0, q_rot=0, rotary_cos=0, rotary_sin=0)
  out = [("rotary on", {}, {}), ("rotary off", dict(_NO_ROTARY), {}), ("NeoX pairs, causal, fp16", dict(rotary_interleaved=0, causal=1, dtype=1), {}),
         ("no new rows", no_rows, {}), ("no new rows, rotary off", {**no_rows, **_NO_ROTARY}, {}), ("D 1024", dict(head_dim=1024, rotary_dim=1024), {})]
  if u:
    out += [("seqlen_q 0: no q needed", dict(seqlen_q=0, q=0, q_rot=0), {}), ("seqlen_q 0, seqlen_new 0: nothing needed", dict(seqlen_q=0, seqlen_new=0, q=0, q_rot=0, k=0, v=0,
                                                                                                                               rotary_cos=0, rotary_sin=0), {})]
  else:
    out += [("positions", dict(positions=POS), {}), ("positions, no rows", dict(positions=POS, **no_rows), {})]
  return out


def calls() -> "list[dict]":
  """Every call of the list, without ``got``: per export and cache form the single faults, one call per two neighbouring checks (both broken) and the accepted calls."""
  out = []
  for export in EXPORTS:
    for paged in (False, True):
      def call(why, params, kv):
        c = {"export": export, "paged": paged, "why": why}
        c.update({"params": params} if params is None or params else {})
        c.update({"kv": kv} if kv and paged else {})
        return c

      chain = check_order(export, paged)
      out += [call(*f) for f in chain + more_faults(export, paged)]
      for (w1, p1, k1), (w2, p2, k2) in zip(chain, chain[1:]):
        if not (set(p1) & set(p2) or set(k1) & set(k2)):
          out.append(call(f"{w1} + {w2}", {**p1, **p2}, {**k1, **k2}))
      out += [call("accepted: " + w, p, k) for w, p, k in accepted(export)]
  return out


def _at(c: dict) -> str:
  return c["export"][0] + ("p" if c["paged"] else "c")


def pack(rec: "list[dict]") -> "list[dict]":
  out = {}
  for c in rec:
    out.setdefault(json.dumps({k: v for k, v in c.items() if k not in ("export", "paged")}), []).append(_at(c))
  return [{"at": " ".join(at), **json.loads(key)} for key, at in out.items()]


def load(path: str = OUT) -> "list[dict]":
  """The calls of the file one by one (in the file's order, not that of ``calls()``)."""
  with open(path, encoding="utf-8") as f:
    return [{"export": "uniform" if at[0] == "u" else "ragged", "paged": at[1] == "p", **{k: v for k, v in e.items() if k != "at"}}
            for e in json.load(f) for at in e["at"].split()]


def record(lib) -> "list[dict]":
  out = []
  for c in calls():
    got = replay(lib, c)
    assert (got == NO_DEVICE) == c["why"].startswith("accepted"), (c, got)
    out.append({**c, "got": got})
  return out


if __name__ == "__main__":
  ap = argparse.ArgumentParser()
  ap.add_argument("--library", default=None)
  ap.add_argument("--out", default=OUT)
  args = ap.parse_args()
  rec = record(_hip().load_library(args.library))
  with open(args.out, "w", encoding="utf-8") as f:
    f.write("[\n" + ",\n".join(json.dumps(c) for c in pack(rec)) + "\n]\n")
  print(f"{len(rec)} calls ({sum(c['got'] == NO_DEVICE for c in rec)} accepted) -> {args.out}")
