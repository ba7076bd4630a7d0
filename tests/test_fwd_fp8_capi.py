"""The C ABI of the FP8 forward without a GPU: ONE table with a row per ``fail(`` of ``fp8_check_shape``, ``ffpa_attn_fp8_quantize``, ``fp8_fwd_check``,
``ffpa_attn_fp8_fwd`` and ``ffpa_attn_fp8_fwd_kernel`` (csrc/ffpa_capi.hip) — the single faults that reach it, its status, a word of
``ffpa_attn_last_error()`` — counted against the C source by function name, so a refusal added later fails here until it has a row; and what
``ffpa_attn_fp8_codes`` refuses in Python before any launch.  The pointers are fake aligned integers: every refusal returns in front of ``check_device()``."""

import ctypes
import os
import re

import pytest
import torch

from ffpa_attn_amd import ffpa_attn_fp8_codes, hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUANT_POINTERS = ("q", "k", "v", "q8", "k8", "v8t", "q_scale", "k_scale", "v_scale", "workspace")
FWD_POINTERS = ("q8", "k8", "v8t", "q_scale", "k_scale", "v_scale", "o")
BOTH, FWD2 = ("quantize", "fwd", "kernel"), ("fwd", "kernel")


@pytest.fixture(scope="module")
def lib():
  if not hip.library_available():
    from ffpa_attn_amd import build

    build.build()
  return hip.load_library()


def _each(calls, *overs):
  return [(call, over) for call in calls for over in overs]


def _stride(field, i, value):
  return {field: (i, value)}


# (function, status, a word of the message, the single faults [(entry point, what differs from a good call)]); no fault: a report of the launch itself, behind
# check_device() — it needs a device that fails, which no test provokes
TABLE = [
  ("fp8_check_shape", 2, b"dtype 2 is not bf16(0)/fp16(1)", _each(BOTH, dict(dtype=2))),
  ("fp8_check_shape", 3, b"the FP8 forward is built for 256, 320, 384, 448 and 512", _each(BOTH, dict(head_dim=128), dict(head_dim=288), dict(head_dim=576))),
  ("fp8_check_shape", 4, b"must be positive, heads_q a multiple of heads_kv",
   _each(BOTH, dict(batch=0), dict(heads_q=0), dict(heads_kv=0), dict(seqlen_q=0), dict(seqlen_kv=0), dict(heads_q=3, heads_kv=2))),
  ("fp8_check_shape", 4, b"batch * heads_kv = 65536 is more than 65535", _each(BOTH, dict(batch=32768, heads_q=2, heads_kv=2))),
  ("fp8_check_shape", 4, b"more than 2^30 workgroups", _each(BOTH, dict(batch=32767, heads_q=2, heads_kv=2, seqlen_q=64 * 16385))),
  ("ffpa_attn_fp8_quantize", 1, b"params is NULL", [("quantize", None)]),
  ("ffpa_attn_fp8_quantize", 10, b"ffpa_fp8_quantize_params ABI mismatch: size 160", [("quantize", dict(struct_size=160))]),
  ("ffpa_attn_fp8_quantize", 10, b"must be 0", _each(("quantize",), dict(reserved=1), dict(reserved2=1))),
  ("ffpa_attn_fp8_quantize", 4, b"smooth_k=2 must be 0 or 1", [("quantize", dict(smooth_k=2))]),
  ("ffpa_attn_fp8_quantize", 5, b"must be a non-negative multiple of 8 elements",
   _each(("quantize",), *[_stride(f, i, v) for f in ("q_stride", "k_stride", "v_stride") for i, v in ((0, -8), (1, 260), (2, 4))])),
  ("ffpa_attn_fp8_quantize", 1, b"q / k / v, the scratch and the workspace must be non-NULL", _each(("quantize",), *[{f: None} for f in QUANT_POINTERS])),
  ("ffpa_attn_fp8_quantize", 6, b"q / k / v, the scratch and the workspace must be 16-byte aligned", _each(("quantize",), *[{f: 8} for f in QUANT_POINTERS])),
  ("ffpa_attn_fp8_quantize", 8, b"fp8 quantize launch failed", []),
  ("fp8_fwd_check", 1, b"params is NULL", _each(FWD2, None)),
  ("fp8_fwd_check", 10, b"ffpa_fp8_fwd_params ABI mismatch: size 96", _each(FWD2, dict(struct_size=96))),
  ("fp8_fwd_check", 10, b"ffpa_fp8_fwd_params.reserved=7 must be 0", _each(FWD2, dict(reserved=7))),
  ("fp8_fwd_check", 4, b"causal=2 must be 0 or 1", _each(FWD2, dict(causal=2))),
  ("fp8_fwd_check", 5, b"must be a non-negative multiple of 4 elements", _each(FWD2, *[_stride("o_stride", i, v) for i, v in ((0, -4), (1, 258), (2, 2))])),
  ("ffpa_attn_fp8_fwd", 1, b"the scratch and o must be non-NULL", _each(("fwd",), *[{f: None} for f in FWD_POINTERS])),
  ("ffpa_attn_fp8_fwd", 6, b"the scratch and o must be 16-byte aligned", _each(("fwd",), *[{f: 8} for f in FWD_POINTERS])),
  ("ffpa_attn_fp8_fwd", 9, b"no current HIP device", []),
  ("ffpa_attn_fp8_fwd", 8, b"hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed", []),
  ("ffpa_attn_fp8_fwd", 8, b"fp8 forward launch failed", []),
  ("ffpa_attn_fp8_fwd_kernel", 1, b"buf is NULL or empty", [("kernel", dict(buf=None)), ("kernel", dict(n=0))]),
]
FUNCTIONS = ("fp8_check_shape", "ffpa_attn_fp8_quantize", "fp8_fwd_check", "ffpa_attn_fp8_fwd", "ffpa_attn_fp8_fwd_kernel")
_KEEP = []


def _good(call):
  """A call every check accepts: B 2, Hq 4, Hkv 2, (64, 128), D 256, bf16, contiguous, every pointer one fake 16-byte aligned address."""
  buf = (ctypes.c_char * 64)()
  _KEEP.append(buf)
  base = (ctypes.addressof(buf) + 15) & ~15
  cls = hip.FfpaFp8QuantizeParams if call == "quantize" else hip.FfpaFp8FwdParams
  p = hip._stamped(cls)
  for f, t in cls._fields_:
    if t is ctypes.c_void_p:
      setattr(p, f, base)
  p.batch, p.heads_q, p.heads_kv, p.seqlen_q, p.seqlen_kv, p.head_dim, p.dtype = 2, 4, 2, 64, 128, 256, 0
  if call == "quantize":
    p.smooth_k, p.q_premul = 1, 0.09
    for i, (sq, sk) in enumerate(((4 * 64 * 256, 2 * 128 * 256), (64 * 256, 128 * 256), (256, 256))):
      p.q_stride[i], p.k_stride[i], p.v_stride[i] = sq, sk, sk
  else:
    p.causal = 1
    for i, s in enumerate((4 * 64 * 256, 64 * 256, 256)):
      p.o_stride[i] = s
  return p, base


def _run(lib, call, over):
  p, base = _good(call)
  name = ctypes.create_string_buffer(200)
  extra = {"buf": name, "n": len(name)}
  for field, value in (over or {}).items():
    if field in extra:
      extra[field] = value
    elif field.endswith("_stride"):
      getattr(p, field)[value[0]] = value[1]
    elif dict(type(p)._fields_)[field] is ctypes.c_void_p:
      setattr(p, field, None if value is None else base + value)
    else:
      setattr(p, field, value)
  ref = None if over is None else ctypes.byref(p)
  if call == "kernel":
    return lib.ffpa_attn_fp8_fwd_kernel(ref, extra["buf"], extra["n"])
  return (lib.ffpa_attn_fp8_quantize if call == "quantize" else lib.ffpa_attn_fp8_fwd)(ref, None)


FAULTS = [(fn, status, word, call, over) for fn, status, word, faults in TABLE for call, over in faults]


@pytest.mark.parametrize("fn, status, word, call, over", FAULTS, ids=[f"{fn}-{call}-{over}" for fn, _, _, call, over in FAULTS])
def test_every_refusal_and_its_status(lib, fn, status, word, call, over):
  assert _run(lib, call, over) == status, lib.ffpa_attn_last_error()
  assert word in lib.ffpa_attn_last_error(), lib.ffpa_attn_last_error()


def test_the_good_call_passes_every_check(lib):
  """The faults above are SINGLE faults: the call they are made on is refused by nothing but the missing device, and the kernel query answers."""
  name = ctypes.create_string_buffer(200)
  p, _ = _good("kernel")
  assert lib.ffpa_attn_fp8_fwd_kernel(ctypes.byref(p), name, len(name)) == 0 and b"ffpa_fwd_fp8_kernel<256, bf16>" in name.value, lib.ffpa_attn_last_error()
  if not torch.cuda.is_available():
    for call in ("quantize", "fwd"):
      assert _run(lib, call, {}) == 9 and b"device" in lib.ffpa_attn_last_error(), lib.ffpa_attn_last_error()  # FFPA_ERR_NO_DEVICE: check_device()


def _body(src, name):
  m = re.search(r"^(?:static )?int " + name + r"\(.*?\) \{\n(.*?)^\}\n", src, re.M | re.S)
  assert m, name
  return m.group(1)


def test_the_table_has_a_row_per_fail_of_the_c_source():
  src = open(os.path.join(ROOT, "ffpa_attn_amd", "csrc", "ffpa_capi.hip")).read()
  for fn in FUNCTIONS:
    body = _body(src, fn)
    rows = [r for r in TABLE if r[0] == fn]
    assert body.count("fail(") == len(rows), f"{fn}: {body.count('fail(')} fail( calls in the source, {len(rows)} rows in the table"
    # the rows without a fault are exactly the reports behind check_device(), by their text
    head, _, tail = body.partition("check_device()")
    assert tail.count("fail(") == sum(1 for r in rows if not r[3]) and head.count("fail(") == sum(1 for r in rows if r[3]), fn
    assert all(word.decode() in tail for _, _, word, faults in rows if not faults), fn
  # ... and these five are the FP8 section: every function between its heading and the next one
  section = src[src.index("// ---- the FP8 attention forward"):src.index("// ---- the three sparse latent calls over a WIDE pool")]
  assert tuple(re.findall(r"^(?:static )?int (\w+)\(", section, re.M)) == FUNCTIONS


# ----------------------------------------------------------------------------- ffpa_attn_fp8_codes: what Python refuses before the op
def _scratch(D=256, device="meta"):
  s = hip.fp8_scratch_shapes(1, 2, 2, 8, 8, D)
  new = lambda n: torch.empty(s[n], dtype=torch.float32 if n.endswith("scale") else torch.uint8, device=device)
  return [new(n) for n in ("q8", "q_scale", "k8", "k_scale", "v8t", "v_scale")]


@pytest.mark.parametrize("what, exc, word", [
  ("out_dtype", TypeError, "out_dtype must be torch.bfloat16 or torch.float16, got torch.float32"),
  ("q8 rank", ValueError, r"q8 / k8 / v8t must be \[B, H, tiles, bytes\] and v_scale \[B, Hkv, D\]"),
  ("k8 rank", ValueError, r"q8 / k8 / v8t must be \[B, H, tiles, bytes\]"),
  ("v_scale rank", ValueError, r"v_scale \[B, Hkv, D\]"),
  ("head dim", NotImplementedError, "head dim 288 is not built"),
  ("heads", ValueError, "integer multiple of key/value num_heads"),
])
def test_codes_entry_refusals(what, exc, word):
  a = _scratch()
  kw = dict(seqlen_q=8, seqlen_kv=8)
  if what == "out_dtype":
    kw["out_dtype"] = torch.float32
  elif what == "q8 rank":
    a[0] = a[0].flatten(2)
  elif what == "k8 rank":
    a[2] = a[2][0]
  elif what == "v_scale rank":
    a[5] = a[5][:, :, None]
  elif what == "head dim":
    a[5] = torch.empty(1, 2, 288, device="meta")
  elif what == "heads":
    a[0] = torch.empty(1, 3, 1, 64 * 256, dtype=torch.uint8, device="meta")
  with pytest.raises(exc, match=word):
    ffpa_attn_fp8_codes(*a, **kw)
