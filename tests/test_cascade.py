"""Cascade (shared-prefix) attention and the merge of two attention states without a GPU: the merge struct against its ctypes mirror and gcc, every argument
check of ffpa_attn_merge_states (they come before any device work), the merge kernel's ISA, the header == EXPORTS and ABI pins, the refusals of
ffpa_merge_attn_states / ffpa_attn_with_kvcache_cascade and the fake ops on meta tensors, and the cascade=None rule against its measured table."""

import ctypes
import glob
import gzip
import json
import os
import re
import subprocess

import pytest
import torch

from ffpa_attn_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
  if not hip.library_available():
    from ffpa_attn_amd import build

    build.build()
  return hip.load_library()


def test_ctypes_mirror_of_the_merge_params_matches_the_c_header(tmp_path):
  fields = [f[0] for f in hip.FfpaMergeStatesParams._fields_]
  src = tmp_path / "layout.c"
  body = "".join(f'printf("{f} %zu\\n", offsetof(ffpa_merge_states_params, {f}));\n' for f in fields)
  src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ffpa_attn.h"\nint main(void){\n'
                 'printf("sizeof %zu\\n", sizeof(ffpa_merge_states_params));\n'
                 'printf("varlen %zu\\n", sizeof(ffpa_varlen_fwd_params));\nprintf("paged %zu\\n", sizeof(ffpa_paged_kv));\n'
                 'printf("abi %d\\n", FFPA_ATTN_ABI_VERSION);\n' + body + "return 0;}\n")
  exe = tmp_path / "layout"
  subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
  out = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
  assert int(out["sizeof"]) == ctypes.sizeof(hip.FfpaMergeStatesParams) == 144
  for f in fields:
    assert int(out[f]) == getattr(hip.FfpaMergeStatesParams, f).offset, f
  # the existing layouts and the ABI version stay where they were
  assert int(out["varlen"]) == 216 and int(out["paged"]) == 56 and int(out["abi"]) == 7


def test_abi_version_stays_7_and_the_symbol_is_exported(lib):
  assert hip.ABI_VERSION == 7 and lib.ffpa_attn_query(0) == 7
  assert "ffpa_attn_merge_states" in hip.EXPORTS and lib.ffpa_attn_merge_states is not None
  header = open(os.path.join(ROOT, "include", "ffpa_attn.h")).read()
  declared = set(re.findall(r"^\s*(?:int|size_t|const char\*)\s+(ffpa_attn_\w+)\s*\(", header, flags=re.M))
  assert declared == set(hip.EXPORTS)


def _params(**over):
  """A well-formed merge (T 6 tokens, H 4 heads, D 128, contiguous [T, H, D], LSE [H, T]) on a host buffer: only the argument checks run on it — each test
  breaks one argument."""
  p = hip.FfpaMergeStatesParams()
  p.struct_size = ctypes.sizeof(hip.FfpaMergeStatesParams)
  p.abi_version = hip.ABI_VERSION
  buf = (ctypes.c_char * 4096)()
  base = (ctypes.addressof(buf) + 15) & ~15
  p.o_a = p.o_b = p.o = base
  p.lse_a = p.lse_b = p.lse = base + 16
  p.tokens, p.heads, p.head_dim, p.dtype = 6, 4, 128, 0
  p.o_a_stride[:] = p.o_b_stride[:] = p.o_stride[:] = [4 * 128, 128]
  p.lse_a_stride_head = p.lse_b_stride_head = p.lse_stride_head = 6
  for name, value in over.items():
    if name.endswith("_stride"):
      getattr(p, name)[:] = value
    else:
      setattr(p, name, value)
  p._keepalive = buf
  return p


@pytest.mark.parametrize("over, status, text", [
  (dict(struct_size=136), 10, b"ffpa_merge_states_params ABI mismatch"),
  (dict(abi_version=6), 10, b"ABI mismatch"),
  (dict(dtype=2), 2, b"dtype"),
  (dict(dtype=-1), 2, b"dtype"),
  (dict(tokens=-1), 4, b"negative"),
  (dict(heads=-2), 4, b"negative"),
  (dict(head_dim=100), 3, b"headdim not support"),
  (dict(head_dim=0), 3, b"headdim not support"),
  (dict(head_dim=1032), 3, b"headdim not support"),
  (dict(o_a=None), 1, b"o_a"),
  (dict(o_b=None), 1, b"o_b"),
  (dict(o=None), 1, b"non-NULL"),
  (dict(lse_a=None), 1, b"lse_a"),
  (dict(lse_b=None), 1, b"lse_b"),
  (dict(o_a_stride=[512, -128]), 5, b"negative"),
  (dict(o_b_stride=[516, 128]), 5, b"multiple of 8"),
  (dict(o_stride=[512, 124]), 5, b"multiple of 8"),
  (dict(o_stride=[128, 128]), 5, b"overlap"),
  (dict(o_stride=[512, 64]), 5, b"overlap"),
  (dict(lse_a_stride_head=-6), 5, b"negative"),
  (dict(lse_stride_head=5), 5, b"lse head stride"),
])
def test_status_codes_of_the_merge_come_before_any_device_work(lib, over, status, text):
  p = _params(**over)
  assert lib.ffpa_attn_merge_states(ctypes.byref(p), None) == status
  assert text in lib.ffpa_attn_last_error(), lib.ffpa_attn_last_error()


def test_misaligned_pointers_of_the_merge(lib):
  for name, add in (("o_a", 8), ("o_b", 2), ("o", 4), ("lse_a", 2), ("lse_b", 1), ("lse", 2)):
    p = _params()
    setattr(p, name, getattr(p, name) + add)
    assert lib.ffpa_attn_merge_states(ctypes.byref(p), None) == 6, name
    assert b"aligned" in lib.ffpa_attn_last_error()
  assert lib.ffpa_attn_merge_states(None, None) == 1


def test_what_the_merge_does_not_need_is_not_checked(lib):
  # Every call here returns before any device work — a refusal by a check placed AFTER the one under test, or an empty merge (0 tokens or 0 heads), which
  # returns before the device is even looked up — so this runs the same on a machine with or without a GPU and never launches on the host buffer.
  # no output LSE: its (negative) stride is not read — the call is refused by the later overlap check of o instead
  p = _params(lse=None, lse_stride_head=-1, o_stride=[128, 128])
  assert lib.ffpa_attn_merge_states(ctypes.byref(p), None) == 5 and b"overlap" in lib.ffpa_attn_last_error(), lib.ffpa_attn_last_error()
  for over in (dict(tokens=0), dict(heads=0), dict(tokens=0, lse=None, lse_stride_head=-1)):
    p = _params(**over)
    assert lib.ffpa_attn_merge_states(ctypes.byref(p), None) == 0, over
  # at most one token and one head: strides that would overlap two rows are not refused (empty merges, so nothing is launched)
  for over in (dict(tokens=1, heads=0), dict(tokens=0, heads=1)):
    p = _params(o_stride=[0, 0], lse_stride_head=0, **over)
    assert lib.ffpa_attn_merge_states(ctypes.byref(p), None) == 0, over
  # ... and with two heads the same strides are
  p = _params(tokens=1, heads=2, o_stride=[0, 0], lse_stride_head=1)
  assert lib.ffpa_attn_merge_states(ctypes.byref(p), None) == 5 and b"overlap" in lib.ffpa_attn_last_error()


def test_merge_kernel_isa_moves_16_byte_rows_without_scratch():
  """The merge kernel's device assembly (build() keeps it, gzip-compressed, in csrc/build/temps_merge): both dtypes move O with 16-byte loads and stores, use no
  scratch and spill nothing; the only narrower accesses are the LSEs (one dword each)."""
  paths = glob.glob(os.path.join(ROOT, "ffpa_attn_amd", "csrc", "build", "temps_merge", "*gfx950.s*"))
  if not paths:
    pytest.skip("no device assembly in csrc/build/temps_merge (python -m ffpa_attn_amd.build keeps it)")
  path = paths[0]
  text = (gzip.open(path, "rt") if path.endswith(".gz") else open(path)).read()
  kernels = re.findall(r"^(_Z\w*ffpa_merge_states_kernel\w*):", text, flags=re.M)
  assert len(kernels) == 2, kernels
  for k in kernels:
    body = text.split(f"\n{k}:", 1)[1].split(".Lfunc_end", 1)[0]
    assert "scratch_" not in body and "buffer_store" not in body, k
    loads = re.findall(r"global_load_(dword\w*)", body)
    stores = re.findall(r"global_store_(dword\w*)", body)
    assert loads.count("dwordx4") == 2 and stores.count("dwordx4") == 1, (k, loads, stores)
    assert sorted(loads) == ["dword", "dword", "dwordx4", "dwordx4"] and sorted(stores) == ["dword", "dwordx4"], (k, loads, stores)
    # memory is written through vector stores only
    assert not re.search(r"^\s+s_\w*(store|atomic)", body, flags=re.M | re.I), k
  meta = re.findall(r"\.name:\s+(_Z\w*ffpa_merge_states_kernel\w*)(.*?)\.wavefront_size", text, flags=re.S)
  assert len(meta) == 2
  for name, block in meta:
    assert re.search(r"\.private_segment_fixed_size:\s+0\b", block), name
    assert re.search(r"\.vgpr_spill_count:\s+0\b", block) and re.search(r"\.sgpr_spill_count:\s+0\b", block), name


# ---- the public calls on meta tensors: everything they refuse, they refuse before touching a device
def _meta(*shape, dtype=torch.bfloat16):
  return torch.empty(*shape, dtype=dtype, device="meta")


def _merge_args(T=5, H=4, D=128, dtype=torch.bfloat16):
  return dict(o_a=_meta(T, H, D, dtype=dtype), lse_a=_meta(H, T, dtype=torch.float32), o_b=_meta(T, H, D, dtype=dtype), lse_b=_meta(H, T, dtype=torch.float32))


@pytest.mark.parametrize("kw, exc, text", [
  (dict(o_b=_meta(5, 4, 128, dtype=torch.float16)), TypeError, "one dtype"),
  (dict(o_a=_meta(5, 4, 128, dtype=torch.float32), o_b=_meta(5, 4, 128, dtype=torch.float32)), TypeError, "fp16/bf16"),
  (dict(lse_a=_meta(4, 5, dtype=torch.bfloat16)), TypeError, "float32"),
  (dict(o_b=_meta(5, 4, 64)), ValueError, "one shape"),
  (dict(o_a=_meta(5, 512), o_b=_meta(5, 512)), ValueError, "tokens, heads, head_dim"),
  (dict(o_a=_meta(5, 4, 100), o_b=_meta(5, 4, 100)), ValueError, "multiple of 8"),
  (dict(o_a=_meta(5, 4, 1032), o_b=_meta(5, 4, 1032)), ValueError, "multiple of 8"),
  (dict(lse_a=_meta(5, 4, dtype=torch.float32)), ValueError, r"lse_a must be \[heads=4, tokens=5\]"),
  (dict(lse_b=_meta(4, 6, dtype=torch.float32)), ValueError, "lse_b must be"),
  (dict(lse_b=torch.empty(4, 5)), ValueError, "device"),
  (dict(o_b=None), TypeError, "o_b must be a tensor"),
])
def test_merge_host_checks(kw, exc, text):
  from ffpa_attn_amd import ffpa_merge_attn_states

  args = _merge_args()
  args.update(kw)
  with pytest.raises(exc, match=text):
    ffpa_merge_attn_states(**args)


def test_merge_is_inference_only():
  from ffpa_attn_amd import ffpa_merge_attn_states

  args = _merge_args()
  args["o_b"] = torch.empty(5, 4, 128, dtype=torch.bfloat16, device="meta", requires_grad=True)
  with pytest.raises(NotImplementedError, match="inference only: o_b requires grad"):
    ffpa_merge_attn_states(**args)
  with torch.no_grad():
    o, lse = ffpa_merge_attn_states(**args)
  assert o.shape == (5, 4, 128)


@pytest.mark.parametrize("T, H, D, dtype", [(1, 1, 8, torch.bfloat16), (7, 32, 512, torch.float16), (0, 4, 1024, torch.bfloat16)])
def test_fake_merge_op_shapes_on_meta(T, H, D, dtype):
  import ffpa_attn_amd.hip  # noqa: F401  (registers the op)

  a = _merge_args(T, H, D, dtype)
  o, lse = torch.ops.ffpa_attn._merge_states_hip(a["o_a"], a["lse_a"], a["o_b"], a["lse_b"])
  assert o.shape == (T, H, D) and o.dtype == dtype and lse.shape == (H, T) and lse.dtype == torch.float32
  from ffpa_attn_amd import ffpa_merge_attn_states

  o2, lse2 = ffpa_merge_attn_states(**a)
  assert o2.shape == o.shape and lse2.shape == lse.shape


def test_merge_has_no_cpu_kernel():
  from ffpa_attn_amd import ffpa_merge_attn_states

  with pytest.raises(NotImplementedError):
    ffpa_merge_attn_states(torch.zeros(2, 2, 8, dtype=torch.bfloat16), torch.zeros(2, 2), torch.zeros(2, 2, 8, dtype=torch.bfloat16), torch.zeros(2, 2))


def _cascade(**kw):
  from ffpa_attn_amd import ffpa_attn_with_kvcache_cascade

  args = dict(q=_meta(4, 1, 32, 128), k_cache=_meta(64, 64, 8, 128), v_cache=_meta(64, 64, 8, 128), cache_seqlens=_meta(4, dtype=torch.int32),
              block_table=_meta(4, 8, dtype=torch.int32), shared_prefix_len=256)
  args.update(kw)
  return ffpa_attn_with_kvcache_cascade(**args)


_CASCADE_REFUSALS = [
  (dict(shared_prefix_len=-64), ValueError, "non-negative"),
  (dict(shared_prefix_len=64.0), TypeError, "shared_prefix_len must be an int"),
  (dict(shared_prefix_len=True), TypeError, "shared_prefix_len must be an int"),
  (dict(shared_prefix_len=None), TypeError, "shared_prefix_len must be an int"),
  (dict(shared_prefix_len=100), ValueError, "multiple of page_size"),
  (dict(shared_prefix_len=576), ValueError, "exceeds the cache capacity"),
  (dict(cascade=1), TypeError, "cascade must be True, False or None"),
  (dict(cascade="auto"), TypeError, "cascade must be"),
  # ffpa_attn_with_kvcache's own checks, on every route
  (dict(q=_meta(4, 1, 32, 64)), ValueError, "head dim of the cache"),
  (dict(q=_meta(4, 1, 30, 128)), ValueError, "multiple of key/value num_heads"),
  (dict(block_table=_meta(3, 8, dtype=torch.int32)), ValueError, "block_table"),
  (dict(cache_seqlens=_meta(5, dtype=torch.int32)), ValueError, "cache_seqlens"),
  (dict(k=_meta(4, 1, 8, 128), v=_meta(4, 2, 8, 128)), ValueError, "share their shape"),
  (dict(q=_meta(4, 1, 32, 128, dtype=torch.float16)), TypeError, "fp16/bf16"),
  (dict(num_splits=-1), ValueError, "num_splits"),
]


# (the cascade argument's own refusals run with cascade set to the bad value; every other refusal under each of None / True / False)
@pytest.mark.parametrize("kw, exc, text, mode", [(kw, exc, text, mode) for kw, exc, text in _CASCADE_REFUSALS for mode in (None, True, False)
                                                 if not ("cascade" in kw and mode is False)])
def test_cascade_host_checks(kw, exc, text, mode):
  with pytest.raises(exc, match=text):
    _cascade(**{"cascade": mode, **kw})


def test_cascade_checks_a_contiguous_prefix_against_the_capacity():
  kc = _meta(4, 300, 8, 128)
  with pytest.raises(ValueError, match="exceeds the cache capacity"):
    _cascade(k_cache=kc, v_cache=kc, block_table=None, shared_prefix_len=301)
  with pytest.raises(NotImplementedError):  # (no page-size rule without a table; the contiguous launch itself needs a GPU tensor)
    _cascade(k_cache=kc, v_cache=kc, block_table=None, shared_prefix_len=100, cascade=True)


@pytest.mark.parametrize("mode", [None, True, False])
def test_cascade_is_inference_only(mode):
  with pytest.raises(NotImplementedError, match="inference only"):
    _cascade(q=torch.empty(4, 1, 32, 128, dtype=torch.bfloat16, device="meta", requires_grad=True), cascade=mode)


def test_cascade_has_no_unsupported_options_in_its_signature():
  import inspect

  from ffpa_attn_amd import ffpa_attn_with_kvcache_cascade

  params = inspect.signature(ffpa_attn_with_kvcache_cascade).parameters
  assert list(params)[:9] == ["q", "k_cache", "v_cache", "k", "v", "rotary_cos", "rotary_sin", "cache_seqlens", "block_table"]
  for name in ("shared_prefix_len", "softmax_scale", "causal", "rotary_interleaved", "num_splits", "return_softmax_lse", "cascade"):
    assert params[name].kind is inspect.Parameter.KEYWORD_ONLY, name
  for name in ("cache_batch_idx", "cache_leftpad", "window_size", "softcap", "alibi_slopes"):
    assert name not in params
  with pytest.raises(TypeError):
    _cascade(window_size=(64, 0))


@pytest.mark.parametrize("mode", [None, True, False])
@pytest.mark.parametrize("rotary", [False, True])
def test_cascade_shapes_on_meta(mode, rotary):
  """The paged route end to end on meta tensors (every launch is a registered op with a fake): the append, both passes and the merge."""
  q = _meta(3, 4, 32, 512)
  pool = _meta(40, 128, 8, 512)
  bt = _meta(3, 5, dtype=torch.int32)
  k = _meta(3, 4, 8, 512)
  cos = _meta(640, 64) if rotary else None
  used = _meta(3, dtype=torch.int32)
  out, lse = _cascade(q=q, k_cache=pool, v_cache=pool, k=k, v=k, rotary_cos=cos, rotary_sin=cos, cache_seqlens=used, block_table=bt, shared_prefix_len=256,
                      causal=True, return_softmax_lse=True, cascade=mode)
  assert out.shape == (3, 4, 32, 512) and out.dtype == torch.bfloat16 and lse.shape == (3, 32, 4) and lse.dtype == torch.float32
  out = _cascade(q=q, k_cache=pool, v_cache=pool, cache_seqlens=used, block_table=bt, shared_prefix_len=0, cascade=mode)
  assert out.shape == (3, 4, 32, 512)


def test_public_names():
  import ffpa_attn_amd

  assert "ffpa_attn_with_kvcache_cascade" in ffpa_attn_amd.__all__ and "ffpa_merge_attn_states" in ffpa_attn_amd.__all__


# ---- the cascade=None rule
def test_cascade_rule_table():
  from ffpa_attn_amd.kvcache import cascade_rule

  # never for a batch of one or without a shared prefix
  for args in ((1, 1, 32, 8, 512, 32768, 64), (1, 4, 32, 8, 1024, 32768, 64), (64, 1, 32, 8, 512, 0, 64), (64, 4, 16, 4, 1024, 0, 64)):
    assert cascade_rule(*args) is False, args
  # (B, Sq, Hq, Hkv, D, P, page) -> taken: the re-reads saved, (B - 1) x P x Hkv x D x 4 bytes, reach 1 GiB inside the measured envelope (Sq <= 4, D >= 512)
  table = [
    ((64, 1, 32, 8, 512, 2048, 64), True),   # 2016 MiB saved
    ((16, 4, 32, 8, 512, 8192, 64), True),   # 1920 MiB
    ((4, 1, 16, 4, 1024, 32768, 64), True),  # 1536 MiB
    ((4, 4, 32, 8, 512, 32768, 256), True),
    ((16, 1, 32, 8, 512, 2048, 64), False),  # 480 MiB
    ((4, 1, 32, 8, 512, 8192, 64), False),   # 384 MiB
    ((9, 1, 32, 8, 512, 8192, 64), True),    # exactly 1 GiB
    ((8, 1, 32, 8, 512, 8192, 64), False),   # 896 MiB
    ((64, 8, 32, 8, 512, 32768, 64), False),  # Sq past the measured envelope
    ((64, 1, 32, 8, 256, 32768, 64), False),  # D below it
    ((64, 0, 32, 8, 512, 32768, 64), False),  # no query token
    ((64, 1, 32, 8, 512, 32768, 0), False),  # a contiguous cache: not measured
    ((64, 1, 8, 8, 512, 32768, 64), False),  # MHA: not measured
    ((64, 1, 16, 8, 512, 32768, 64), False),  # a group of 2: not measured
    ((16, 1, 64, 8, 512, 8192, 64), True),  # a group of 8 (a check row of the profile)
  ]
  for args, taken in table:
    assert cascade_rule(*args) is taken, args
  for row in _measured_rows():
    assert isinstance(cascade_rule(row["B"], row["Sq"], row["Hq"], row["Hkv"], row["D"], row["P"], row["page"]), bool)


def _measured_rows():
  with open(os.path.join(ROOT, "profiles", "r09_cascade_ab.json")) as f:
    return json.load(f)["rows"]


def test_cascade_rule_never_takes_a_measured_loss():
  """Every shape of the committed A/B (tools/gpu_cascade_ab.py on MI355X): where the rule takes the cascade, the cascade was faster, replayed from a graph
  and launched eagerly."""
  from ffpa_attn_amd.kvcache import cascade_rule

  rows = _measured_rows()
  assert len(rows) >= 30
  taken = 0
  for r in rows:
    if cascade_rule(r["B"], r["Sq"], r["Hq"], r["Hkv"], r["D"], r["P"], r["page"]):
      taken += 1
      assert r["us"]["cascade"] < r["us"]["plain"] and r["us"]["cascade eager"] < r["us"]["plain eager"], r
  assert taken > 0
