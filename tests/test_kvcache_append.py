"""The KV-cache append + rotary without a GPU: the C struct against its ctypes mirror, every argument check of ffpa_attn_kvcache_append (they come before any
device work), the append kernel's ISA, and ffpa_attn_with_kvcache(k=, v=, rotary_cos=, rotary_sin=)'s host-side checks and fake op on meta tensors."""

import ctypes
import glob
import gzip
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


def test_ctypes_mirror_of_the_append_params_matches_the_c_header(tmp_path):
  fields = [f[0] for f in hip.FfpaKvAppendParams._fields_]
  src = tmp_path / "layout.c"
  body = "".join(f'printf("{f} %zu\\n", offsetof(ffpa_kv_append_params, {f}));\n' for f in fields)
  src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ffpa_attn.h"\nint main(void){\n'
                 'printf("sizeof %zu\\n", sizeof(ffpa_kv_append_params));\n' + body + "return 0;}\n")
  exe = tmp_path / "layout"
  subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
  out = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
  assert int(out["sizeof"]) == ctypes.sizeof(hip.FfpaKvAppendParams) == 280
  for f in fields:
    assert int(out[f]) == getattr(hip.FfpaKvAppendParams, f).offset, f


def test_abi_version_stays_7_and_the_symbol_is_exported(lib):
  assert hip.ABI_VERSION == 7 and lib.ffpa_attn_query(0) == 7
  assert "ffpa_attn_kvcache_append" in hip.EXPORTS and lib.ffpa_attn_kvcache_append is not None


def _params(**over):
  """A well-formed decode call (B 3, Hq 8 / Hkv 2, D 512, 1 new token, NeoX rotary over 128 dims, contiguous cache of 1024) on a host buffer: only the argument
  checks run on it — each test breaks one argument."""
  p = hip.FfpaKvAppendParams()
  p.struct_size = ctypes.sizeof(hip.FfpaKvAppendParams)
  p.abi_version = hip.ABI_VERSION
  buf = (ctypes.c_char * 4096)()
  base = (ctypes.addressof(buf) + 15) & ~15
  p.q = p.k = p.v = p.k_cache = p.v_cache = p.q_rot = p.rotary_cos = p.rotary_sin = base
  p.seqused, p.cache_seqlens = base + 16, base + 32
  p.batch, p.heads_q, p.heads_kv, p.head_dim = 3, 8, 2, 512
  p.seqlen_q, p.seqlen_new, p.capacity, p.seqlen_ro = 1, 1, 1024, 1024
  p.q_stride[:] = p.q_rot_stride[:] = [8 * 512, 8 * 512, 512]
  p.k_stride[:] = p.v_stride[:] = [2 * 512, 2 * 512, 512]
  p.k_cache_stride[:] = p.v_cache_stride[:] = [1024 * 2 * 512, 2 * 512, 512]
  p.rotary_dim, p.rotary_interleaved, p.causal, p.dtype = 128, 0, 1, 0
  for name, value in over.items():
    if name.endswith("_stride"):
      getattr(p, name)[:] = value
    else:
      setattr(p, name, value)
  p._keepalive = buf
  return p


def _pool(p, **over):
  kv = hip.FfpaPagedKv()
  kv.struct_size = ctypes.sizeof(hip.FfpaPagedKv)
  kv.block_table = p.cache_seqlens
  kv.pages_per_row, kv.page_size, kv.num_pages, kv.bt_stride = 16, 64, 48, 16
  kv.k_page_stride = kv.v_page_stride = 64 * 2 * 512
  for name, value in over.items():
    setattr(kv, name, value)
  return kv


@pytest.mark.parametrize("over, status, text", [
  (dict(struct_size=272), 10, b"ffpa_kv_append_params ABI mismatch"),
  (dict(abi_version=6), 10, b"ABI mismatch"),
  (dict(dtype=2), 2, b"dtype"),
  (dict(batch=0), 4, b"non-positive"),
  (dict(heads_kv=3), 4, b"num_heads"),
  (dict(head_dim=100), 3, b"headdim not support"),
  (dict(head_dim=1032), 3, b"headdim not support"),
  (dict(seqlen_new=-1), 4, b"negative"),
  (dict(seqlen_q=-2), 4, b"negative"),
  (dict(capacity=0), 4, b"capacity"),
  (dict(rotary_dim=24), 4, b"rotary_dim"),
  (dict(rotary_dim=528), 4, b"rotary_dim"),
  (dict(rotary_dim=-16), 4, b"rotary_dim"),
  (dict(seqlen_ro=1023), 4, b"seqlen_ro"),
  (dict(k_cache=None), 1, b"k_cache"),
  (dict(seqused=None), 1, b"seqused"),
  (dict(cache_seqlens=None), 1, b"cache_seqlens"),
  (dict(k=None), 1, b"k / v"),
  (dict(v=None), 1, b"k / v"),
  (dict(q_rot=None), 1, b"q_rot"),
  (dict(rotary_sin=None), 1, b"rotary_sin"),
  # an append without query rows still reads the tables for the rotated K rows
  (dict(seqlen_q=0, rotary_cos=None), 1, b"rotary_cos"),
  (dict(seqlen_q=0, q=None, q_rot=None, rotary_sin=None), 1, b"rotary_sin"),
  (dict(k_stride=[1024, -1024, 512]), 5, b"negative"),
  (dict(v_cache_stride=[1024 * 2 * 512, 2 * 512 + 4, 512]), 5, b"multiple of 8"),
  (dict(q_rot_stride=[4096, 4096, 500]), 5, b"multiple of 8"),
])
def test_status_codes_of_the_append_come_before_any_device_work(lib, over, status, text):
  p = _params(**over)
  assert lib.ffpa_attn_kvcache_append(ctypes.byref(p), None, None) == status
  assert text in lib.ffpa_attn_last_error(), lib.ffpa_attn_last_error()


def test_misaligned_and_aliased_pointers_of_the_append(lib):
  for name, add in (("k_cache", 8), ("v", 8), ("q", 8), ("q_rot", 4), ("rotary_cos", 8), ("seqused", 2), ("cache_seqlens", 1)):
    p = _params()
    setattr(p, name, getattr(p, name) + add)
    assert lib.ffpa_attn_kvcache_append(ctypes.byref(p), None, None) == 6, name
    assert b"aligned" in lib.ffpa_attn_last_error()
  p = _params()
  p.seqused = p.cache_seqlens
  assert lib.ffpa_attn_kvcache_append(ctypes.byref(p), None, None) == 4 and b"seqused" in lib.ffpa_attn_last_error()
  assert lib.ffpa_attn_kvcache_append(None, None, None) == 1
  # K rows only (seqlen_q = 0): the tables are still read, so their alignment is still checked
  for name in ("rotary_cos", "rotary_sin"):
    p = _params(seqlen_q=0, q=None, q_rot=None)
    setattr(p, name, getattr(p, name) + 8)
    assert lib.ffpa_attn_kvcache_append(ctypes.byref(p), None, None) == 6 and b"aligned" in lib.ffpa_attn_last_error(), name


def test_paged_attention_call_keeps_its_order_of_checks(lib):
  # the pool checks the append shares with ffpa_attn_varlen_paged_fwd: a NULL seqused_kv is still reported before the rest of the pool's checks
  p = hip.FfpaVarlenFwdParams()
  p.struct_size = ctypes.sizeof(hip.FfpaVarlenFwdParams)
  p.abi_version = hip.ABI_VERSION
  buf = (ctypes.c_char * 4096)()
  base = (ctypes.addressof(buf) + 15) & ~15
  p.q = p.k = p.v = p.o = p.cu_seqlens_q = base
  p.batch, p.heads_q, p.heads_kv, p.head_dim, p.max_seqlen_q, p.max_seqlen_kv = 3, 8, 2, 512, 1, 2000
  p.q_stride[:] = p.o_stride[:] = [8 * 512, 512]
  p.k_stride[:] = p.v_stride[:] = [2 * 512, 512]
  p.softmax_scale, p.rescale_threshold = 512 ** -0.5, -1.0
  kv = hip.FfpaPagedKv()
  kv.struct_size = ctypes.sizeof(hip.FfpaPagedKv)
  kv.block_table = base + 2  # (misaligned, and page_size 32: both come after seqused_kv)
  kv.pages_per_row, kv.page_size, kv.num_pages, kv.bt_stride = 32, 32, 96, 32
  assert lib.ffpa_attn_varlen_paged_fwd(ctypes.byref(p), ctypes.byref(kv), None) == 1 and b"seqused_kv" in lib.ffpa_attn_last_error()


def test_what_the_append_does_not_need_is_not_checked(lib):
  # seqlen_new = 0: k / v may be NULL (and their strides anything); no rotary: q / q_rot / cos / sin and seqlen_ro are not read.  Each call is then refused by
  # a check placed after these (the seqused / cache_seqlens alias), never by a check of what it does not need.
  p = _params(seqlen_new=0, k=None, v=None, k_stride=[1, 1, 1])
  p.seqused = p.cache_seqlens
  assert lib.ffpa_attn_kvcache_append(ctypes.byref(p), None, None) == 4 and b"seqused must not" in lib.ffpa_attn_last_error()
  p = _params(rotary_dim=0, q=None, q_rot=None, rotary_cos=None, rotary_sin=None, seqlen_ro=0, q_stride=[3, 3, 3])
  p.seqused = p.cache_seqlens
  assert lib.ffpa_attn_kvcache_append(ctypes.byref(p), None, None) == 4 and b"seqused must not" in lib.ffpa_attn_last_error()
  p = _params(seqlen_q=0, q=None, q_rot=None, q_stride=[3, 3, 3], q_rot_stride=[3, 3, 3])  # (rotary on, no query rows: q / q_rot are not read)
  p.seqused = p.cache_seqlens
  assert lib.ffpa_attn_kvcache_append(ctypes.byref(p), None, None) == 4 and b"seqused must not" in lib.ffpa_attn_last_error()


@pytest.mark.parametrize("kv_over, status, text", [
  (dict(struct_size=48), 10, b"ffpa_paged_kv ABI mismatch"),
  (dict(block_table=None), 1, b"block_table"),
  (dict(page_size=32), 4, b"page_size"),
  (dict(num_pages=0), 4, b"num_pages"),
  (dict(bt_stride=8), 5, b"bt_stride"),
  (dict(k_page_stride=-8), 5, b"negative"),
])
def test_status_codes_of_the_paged_append(lib, kv_over, status, text):
  p = _params()
  kv = _pool(p, **kv_over)
  assert lib.ffpa_attn_kvcache_append(ctypes.byref(p), ctypes.byref(kv), None) == status
  assert text in lib.ffpa_attn_last_error(), lib.ffpa_attn_last_error()


def test_paged_append_takes_its_capacity_from_the_pool(lib):
  # (capacity is ignored when paged: pages_per_row x page_size = 1024 keys, and seqlen_ro must cover them)
  p = _params(capacity=0, seqlen_ro=1000)
  assert lib.ffpa_attn_kvcache_append(ctypes.byref(p), ctypes.byref(_pool(p)), None) == 4 and b"capacity 1024" in lib.ffpa_attn_last_error()


def test_append_kernel_isa_moves_16_byte_rows_without_scratch():
  """The append kernel's device assembly (build() keeps it, gzip-compressed, in csrc/build/temps_append): every instantiation (bf16 / fp16 x interleaved / NeoX)
  moves K / V / q rows with 16-byte loads and stores, uses no scratch and spills nothing."""
  paths = glob.glob(os.path.join(ROOT, "ffpa_attn_amd", "csrc", "build", "temps_append", "*gfx950.s*"))
  if not paths:
    pytest.skip("no device assembly in csrc/build/temps_append (python -m ffpa_attn_amd.build keeps it)")
  path = paths[0]
  text = (gzip.open(path, "rt") if path.endswith(".gz") else open(path)).read()
  kernels = re.findall(r"^(_Z\w*ffpa_kv_append_kernel\w*):", text, flags=re.M)
  assert len(kernels) == 4, kernels
  for k in kernels:
    body = text.split(f"\n{k}:", 1)[1].split(".Lfunc_end", 1)[0]
    assert "scratch_" not in body and "buffer_store" not in body, k
    loads = re.findall(r"global_load_(dword\w*)", body)
    stores = re.findall(r"global_store_(dword\w*)", body)
    assert loads.count("dwordx4") >= 2 and stores.count("dwordx4") >= 2, (k, loads, stores)
    # the only narrower accesses: the length (one dword in, one out) and the interleaved form's 8-byte cos / sin
    assert all(w in ("dword", "dwordx2", "dwordx4") for w in loads + stores), (k, loads, stores)
    assert stores.count("dword") <= 1, (k, stores)
  meta = re.findall(r"\.name:\s+(_Z\w*ffpa_kv_append_kernel\w*)(.*?)\.wavefront_size", text, flags=re.S)
  assert len(meta) == 4
  for name, block in meta:
    assert re.search(r"\.private_segment_fixed_size:\s+0\b", block), name
    assert re.search(r"\.vgpr_spill_count:\s+0\b", block) and re.search(r"\.sgpr_spill_count:\s+0\b", block), name


# ---- the public call on meta tensors: everything it refuses, it refuses before touching a device
def _meta(*shape, dtype=torch.bfloat16):
  return torch.empty(*shape, dtype=dtype, device="meta")


def _call(**kw):
  from ffpa_attn_amd import ffpa_attn_with_kvcache

  args = dict(q=_meta(2, 1, 32, 128), k_cache=_meta(2, 256, 8, 128), v_cache=_meta(2, 256, 8, 128), k=_meta(2, 1, 8, 128), v=_meta(2, 1, 8, 128),
              cache_seqlens=_meta(2, dtype=torch.int32))
  args.update(kw)
  return ffpa_attn_with_kvcache(**args)


@pytest.mark.parametrize("kw, exc, text", [
  (dict(v=_meta(2, 2, 8, 128)), ValueError, "share their shape"),
  (dict(k=_meta(2, 1, 8, 128, dtype=torch.float16), v=_meta(2, 1, 8, 128, dtype=torch.float16)), TypeError, "dtype"),
  (dict(k=_meta(2, 1, 4, 128), v=_meta(2, 1, 4, 128)), ValueError, "Hkv=8"),
  (dict(k=_meta(3, 1, 8, 128), v=_meta(3, 1, 8, 128)), ValueError, "B=2"),
  (dict(k=_meta(2, 1, 8, 64), v=_meta(2, 1, 8, 64)), ValueError, "D=128"),
  (dict(k=_meta(2, 1, 8, 256)[..., ::2], v=_meta(2, 1, 8, 128)), ValueError, "contiguous last dimension"),
  (dict(cache_seqlens=None), ValueError, "cache_seqlens is required"),
  (dict(rotary_cos=_meta(256, 12), rotary_sin=_meta(256, 12)), ValueError, "rotary_dim"),
  (dict(rotary_cos=_meta(256, 72), rotary_sin=_meta(256, 72)), ValueError, "rotary_dim"),
  (dict(rotary_cos=_meta(255, 32), rotary_sin=_meta(255, 32)), ValueError, "seqlen_ro"),
  (dict(rotary_cos=_meta(256, 32, dtype=torch.float32), rotary_sin=_meta(256, 32, dtype=torch.float32)), TypeError, "rotary_cos must have q's dtype"),
  (dict(rotary_cos=_meta(256, 32), rotary_sin=_meta(256, 16)), ValueError, "share their shape"),
  (dict(rotary_cos=_meta(256, 64)[:, ::2], rotary_sin=_meta(256, 32)), ValueError, "contiguous"),
])
def test_append_host_checks(kw, exc, text):
  with pytest.raises(exc, match=text):
    _call(**kw)


def test_paged_append_checks_seqlen_ro_against_the_table():
  # paged capacity: pages_per_seq x page_size = 4 x 64
  pool = _meta(16, 64, 8, 128)
  bt = _meta(2, 4, dtype=torch.int32)
  with pytest.raises(ValueError, match="seqlen_ro"):
    _call(k_cache=pool, v_cache=pool, block_table=bt, rotary_cos=_meta(255, 32), rotary_sin=_meta(255, 32))
  out = _call(k_cache=pool, v_cache=pool, block_table=bt, rotary_cos=_meta(256, 32), rotary_sin=_meta(256, 32))
  assert out.shape == (2, 1, 32, 128)


@pytest.mark.parametrize("kw, names", [
  (dict(v=None), ["k"]),
  (dict(k=None), ["v"]),
  (dict(k=None, v=None, rotary_cos=_meta(256, 32), rotary_sin=_meta(256, 32)), ["rotary_cos", "rotary_sin"]),
  (dict(rotary_cos=_meta(256, 32)), ["rotary_cos"]),
  (dict(rotary_sin=_meta(256, 32)), ["rotary_sin"]),
  (dict(cache_batch_idx=_meta(2, dtype=torch.int32)), ["cache_batch_idx"]),
  (dict(cache_leftpad=_meta(2, dtype=torch.int32)), ["cache_leftpad"]),
  (dict(window_size=(64, 0)), ["window_size"]),
  (dict(softcap=10.0), ["softcap"]),
  (dict(alibi_slopes=_meta(32, dtype=torch.float32)), ["alibi_slopes"]),
])
def test_what_stays_refused_with_append(kw, names):
  with pytest.raises(NotImplementedError) as e:
    _call(**kw)
  for n in names:
    assert n in str(e.value)
  assert "does not support" in str(e.value)


@pytest.mark.parametrize("paged", [False, True])
@pytest.mark.parametrize("rotary", [False, True])
def test_fake_op_and_public_call_shapes_on_meta(paged, rotary):
  import ffpa_attn_amd.hip  # noqa: F401  (registers the op)

  q = _meta(3, 4, 32, 512)
  kc = _meta(40, 128, 8, 512) if paged else _meta(3, 640, 8, 512)
  bt = _meta(3, 5, dtype=torch.int32) if paged else None
  k = _meta(3, 4, 8, 512)
  cos = _meta(640, 64) if rotary else None
  used = _meta(3, dtype=torch.int32)
  q_rot, seqused = torch.ops.ffpa_attn._kvcache_append_hip(q, kc, kc, k, k, used, bt, cos, cos, False, True)
  assert q_rot.shape == ((3, 4, 32, 512) if rotary else (0,)) and q_rot.dtype == torch.bfloat16
  assert seqused.shape == (3,) and seqused.dtype == torch.int32
  if not paged:
    return  # (the contiguous attention launch is no registered op: on meta tensors only the paged route runs end to end)
  out, lse = _call(q=q, k_cache=kc, v_cache=kc, k=k, v=k, cache_seqlens=used, block_table=bt, rotary_cos=cos, rotary_sin=cos, causal=True,
                   return_softmax_lse=True)
  assert out.shape == (3, 4, 32, 512) and lse.shape == (3, 32, 4) and lse.dtype == torch.float32


def test_the_op_schema_marks_the_caches_as_written():
  import ffpa_attn_amd.hip  # noqa: F401

  schema = torch.ops.ffpa_attn._kvcache_append_hip.default._schema
  written = [a.name for a in schema.arguments if a.alias_info is not None and a.alias_info.is_write]
  assert written == ["k_cache", "v_cache"]
