"""The MLA latent-cache entry point without a GPU: the export, every refusal of ``ffpa_attn_with_kvcache_mla`` (they come before any launch), ``ffpa_mla`` against
its ctypes mirror and gcc, the ABI pins, the refusals of ffpa_attn_varlen_mla_fwd (before any device work) and the plan's chunking rule — as a pure function and
as the C plan reports it."""

import ctypes
import math
import os
import re
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ffpa_attn_amd
from ffpa_attn_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALE = 192 ** -0.5


@pytest.fixture(scope="module")
def lib():
  if not hip.library_available():
    from ffpa_attn_amd import build

    build.build()
  return hip.load_library()


# ----------------------------------------------------------------------------- the Python entry
def test_the_entry_point_is_exported():
  from ffpa_attn_amd import ffpa_attn_with_kvcache_mla

  assert "ffpa_attn_with_kvcache_mla" in ffpa_attn_amd.__all__
  assert ffpa_attn_amd.ffpa_attn_with_kvcache_mla is ffpa_attn_with_kvcache_mla
  assert ffpa_attn_amd.kvcache.ffpa_attn_with_kvcache_mla is ffpa_attn_with_kvcache_mla


def _args(B=2, sq=1, hq=16, hkv=1, d=576, page=64, pages=4):
  q = torch.zeros(B, sq, hq, d, dtype=torch.bfloat16)
  pool = torch.zeros(B * pages, page, hkv, d, dtype=torch.bfloat16)
  table = torch.arange(B * pages, dtype=torch.int32).view(B, pages)
  return q, pool, table


def _call(q, pool, table, dv=512, **kw):
  kw.setdefault("cache_seqlens", 7)
  kw.setdefault("softmax_scale", SCALE)
  return ffpa_attn_amd.ffpa_attn_with_kvcache_mla(q, pool, dv, block_table=table, **kw)


def test_a_missing_scale_is_a_type_error_that_says_why():
  q, pool, table = _args()
  for kw in ({}, {"softmax_scale": None}):
    with pytest.raises(TypeError, match=r"softmax_scale is required.*1 / sqrt\(qk_nope_head_dim \+ qk_rope_head_dim\).*not\s+1 / sqrt\(D\)"):
      ffpa_attn_amd.ffpa_attn_with_kvcache_mla(q, pool, 512, cache_seqlens=7, block_table=table, **kw)
  with pytest.raises(TypeError, match="real number"):
    _call(q, pool, table, softmax_scale="0.07")


def test_the_pair_rule_and_the_build_list():
  q, pool, table = _args()
  for dv in (576 + 64, 1024):
    with pytest.raises(ValueError, match="head_dim_v <= D"):
      _call(q, pool, table, dv=dv)
  for dv in (0, -64, 500, 8):
    with pytest.raises(ValueError, match="multiples of 64"):
      _call(q, pool, table, dv=dv)
  with pytest.raises(TypeError, match="head_dim_v must be an int"):
    _call(q, pool, table, dv=512.0)
  # pairs inside the rule that are not built are named
  for d, dv in ((576, 576), (576, 448), (512, 512), (640, 512), (192, 128)):
    q2, pool2, table2 = _args(d=d)
    with pytest.raises(NotImplementedError, match=rf"\({d}, {dv}\) is not built"):
      _call(q2, pool2, table2, dv=dv)
  q3, pool3, table3 = _args(d=520)
  with pytest.raises(ValueError, match="multiples of 64"):
    _call(q3, pool3, table3)
  assert hip.MLA_BUILDS == ((576, 512),)


def test_shape_refusals():
  q, pool, table = _args()
  with pytest.raises(ValueError, match="page_size .96. must be a positive multiple of 64"):
    _call(q, _args(page=128)[1][:, :96], table)
  q5, pool2, _ = _args(hq=5, hkv=2)
  with pytest.raises(ValueError, match=r"num_heads \(5\) must be a multiple of the latent num_heads \(2\)"):
    _call(q5, pool2, table)
  with pytest.raises(ValueError, match="multiple of 64"):  # a contiguous cache of capacity 100
    ffpa_attn_amd.ffpa_attn_with_kvcache_mla(q, torch.zeros(2, 100, 1, 576, dtype=torch.bfloat16), 512, cache_seqlens=7, softmax_scale=SCALE)
  with pytest.raises(ValueError, match="must have q's batch"):
    ffpa_attn_amd.ffpa_attn_with_kvcache_mla(q, torch.zeros(3, 128, 1, 576, dtype=torch.bfloat16), 512, cache_seqlens=7, softmax_scale=SCALE)
  with pytest.raises(TypeError, match="fp16/bf16"):
    _call(q.float(), pool, table)
  with pytest.raises(ValueError, match="block_table must be an int32 tensor"):
    _call(q, pool, table.long())
  with pytest.raises(ValueError, match="num_splits"):
    _call(q, pool, table, num_splits=-1)
  with pytest.raises(ValueError, match="cache_seqlens"):
    _call(q, pool, table, cache_seqlens=torch.zeros(5, dtype=torch.int32))
  with pytest.raises(TypeError):
    ffpa_attn_amd.ffpa_attn_with_kvcache_mla(q, pool, 512, block_table=table, softmax_scale=SCALE)  # (cache_seqlens is required)
  with pytest.raises(ValueError, match=r"kv must be \[B=2, Snew, Hkv=1, D=576\]"):
    _call(q, pool, table, kv=torch.zeros(2, 1, 2, 576, dtype=torch.bfloat16))


def test_a_tensor_that_requires_grad_raises():
  q, pool, table = _args()
  kv = torch.zeros(2, 1, 1, 576, dtype=torch.bfloat16)
  for i in range(3):
    args = [q, pool, kv]
    args[i] = args[i].clone().requires_grad_(True)
    with pytest.raises(NotImplementedError, match="inference only"):
      _call(args[0], args[1], table, kv=args[2])


@pytest.mark.parametrize("kw", [dict(rotary_cos=torch.zeros(256, 32)), dict(rotary_sin=torch.zeros(256, 32)), dict(window_size=(64, 0)), dict(softcap=30.0),
                                dict(tree_mask=torch.ones(1, 1, dtype=torch.bool)), dict(cu_seqlens_q=torch.zeros(3, dtype=torch.int32)),
                                dict(alibi_slopes=torch.zeros(16)), dict(rotary_interleaved=False)])
def test_rotary_window_and_the_other_unserved_keywords_raise_by_name(kw):
  q, pool, table = _args()
  with pytest.raises(NotImplementedError, match=f"does not support: {next(iter(kw))}"):
    _call(q, pool, table, **kw)
  doc = ffpa_attn_amd.ffpa_attn_with_kvcache_mla.__doc__
  for word in ("window_size", "softcap", "tree_mask", "cu_seqlens_q", "rotary_cos", "FP8"):
    assert word in doc


def test_the_op_has_a_fake():
  q = torch.empty(12, 128, 576, dtype=torch.bfloat16, device="meta")
  pool = torch.empty(40, 64, 1, 576, dtype=torch.bfloat16, device="meta")
  i32 = lambda *s: torch.empty(s, dtype=torch.int32, device="meta")
  o, lse = torch.ops.ffpa_attn._mla_fwd_hip(q, pool, 512, i32(4), i32(3), i32(3, 8), None, None, 4, 512, 0.07, 1)
  assert o.shape == (12, 128, 512) and o.dtype == torch.bfloat16 and lse.shape == (128, 12) and lse.dtype == torch.float32


# ----------------------------------------------------------------------------- the C ABI
def test_ctypes_mirror_of_ffpa_mla_matches_the_c_header(tmp_path):
  fields = [f[0] for f in hip.FfpaMla._fields_]
  src = tmp_path / "layout.c"
  body = "".join(f'printf("{f} %zu\\n", offsetof(ffpa_mla, {f}));\n' for f in fields)
  src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ffpa_attn.h"\nint main(void){\n'
                 'printf("sizeof %zu\\n", sizeof(ffpa_mla));\n'
                 'printf("varlen %zu\\n", sizeof(ffpa_varlen_fwd_params));\nprintf("paged %zu\\n", sizeof(ffpa_paged_kv));\n'
                 'printf("window %zu\\n", sizeof(ffpa_window));\nprintf("abi %d\\n", FFPA_ATTN_ABI_VERSION);\n' + body + "return 0;}\n")
  exe = tmp_path / "layout"
  subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
  out = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
  assert int(out["sizeof"]) == ctypes.sizeof(hip.FfpaMla) == 56
  assert fields == ["struct_size", "reserved", "head_dim_v", "seqlen_new", "kv_new", "cache_seqlens", "kv_new_stride"]
  for f in fields:
    assert int(out[f]) == getattr(hip.FfpaMla, f).offset, f
  # the shared parameter structs keep their layout and the ABI version stays where it was
  assert int(out["varlen"]) == ctypes.sizeof(hip.FfpaVarlenFwdParams) == 216 and int(out["paged"]) == ctypes.sizeof(hip.FfpaPagedKv) == 56
  assert int(out["window"]) == ctypes.sizeof(hip.FfpaWindow) == 16 and int(out["abi"]) == 7


MLA_SYMBOLS = ("ffpa_attn_varlen_mla_fwd", "ffpa_attn_varlen_mla_fwd_plan", "ffpa_attn_varlen_mla_fwd_kernel", "ffpa_attn_varlen_mla_fwd_workspace_bytes")


def test_abi_version_stays_7_and_the_symbols_are_exported(lib):
  assert hip.ABI_VERSION == 7 and lib.ffpa_attn_query(0) == 7
  for name in MLA_SYMBOLS:
    assert name in hip.EXPORTS and getattr(lib, name) is not None, name
  header = open(os.path.join(ROOT, "include", "ffpa_attn.h")).read()
  declared = set(re.findall(r"^\s*(?:int|size_t|const char\*)\s+(ffpa_attn_\w+)\s*\(", header, flags=re.M))
  assert declared == set(hip.EXPORTS)


_KEEP = []


def _buf():
  buf = (ctypes.c_char * 4096)()
  _KEEP.append(buf)
  return (ctypes.addressof(buf) + 15) & ~15


def _call_args(d=576, dv=512, sq=1, B=32, hq=128, hkv=1, max_k=4096, causal=False, num_splits=0, flags=0, over=None, mla_over=None, no_mla=False, no_kv=False,
               snew=0):
  """A well-formed latent-cache call on host buffers (only the argument checks and the plan run on it) -> the ctypes arguments (p, kv | None, m | None) + their owners."""
  p = hip._varlen_params(torch.bfloat16, B, hq, hkv, d, sq, max_k, B * sq, [(hq * d, d), (hkv * d, d), (hkv * d, d), (hq * dv, dv)], causal, SCALE, -1.0, flags,
                         num_splits)
  base = _buf()
  p.q = p.k = p.o = p.cu_seqlens_q = p.seqused_kv = base  # (p.v stays NULL: the latent-cache call does not read it)
  p.workspace, p.workspace_bytes = base, 0xFFFFFFFFFFFFFFFF  # (a call that hands the library its scratch: the plan may split)
  for k_, v_ in (over or {}).items():
    setattr(p, k_, v_)
  pages = -(-max_k // 64)
  kv = hip._paged_kv(base, pages, pages, 64, B * pages, 64 * hkv * d, 0)
  m = hip._stamped(hip.FfpaMla)
  m.head_dim_v = dv
  if snew:
    m.seqlen_new, m.kv_new, m.cache_seqlens = snew, base, base + 64
    m.kv_new_stride[:] = [snew * hkv * d, hkv * d, d]
  for k_, v_ in (mla_over or {}).items():
    setattr(m, k_, v_)
  return ctypes.byref(p), (None if no_kv else ctypes.byref(kv)), (None if no_mla else ctypes.byref(m)), (p, kv, m)


@pytest.mark.parametrize("kw, status, text", [
  (dict(no_mla=True), 1, b"mla is NULL"),
  (dict(no_kv=True), 1, b"paged kv is NULL"),
  (dict(mla_over=dict(struct_size=48)), 10, b"ffpa_mla ABI mismatch"),
  (dict(mla_over=dict(struct_size=0)), 10, b"ffpa_mla ABI mismatch"),
  (dict(mla_over=dict(reserved=1)), 10, b"reserved"),
  (dict(dv=0), 4, b"multiples of 64"),
  (dict(dv=500), 4, b"multiples of 64"),
  (dict(dv=640), 4, b"head_dim_v <= head_dim"),
  (dict(dv=-512), 4, b"multiples of 64"),
  (dict(dv=576), 3, b"(576, 576) is not built"),
  (dict(d=512, dv=512), 3, b"(512, 512) is not built"),
  (dict(mla_over=dict(seqlen_new=-1)), 4, b"seqlen_new"),
  (dict(mla_over=dict(seqlen_new=1)), 1, b"kv_new / cache_seqlens must be non-NULL"),
  # the packed call's and the pool's own refusals come first
  (dict(over=dict(dtype=2)), 2, b"dtype"),
  (dict(over=dict(abi_version=6)), 10, b"ffpa_varlen_fwd_params ABI mismatch"),
  (dict(over=dict(struct_size=8)), 10, b"ffpa_varlen_fwd_params ABI mismatch"),
  (dict(hq=5, hkv=2), 4, b"num_heads"),
])
def test_status_codes_of_the_c_call_come_before_any_device_work(lib, kw, status, text):
  p, kv, m, keep = _call_args(**kw)
  for fn, extra in ((lib.ffpa_attn_varlen_mla_fwd, (None,)), (lib.ffpa_attn_varlen_mla_fwd_plan, ((ctypes.c_int * 5)(),)),
                    (lib.ffpa_attn_varlen_mla_fwd_kernel, (ctypes.create_string_buffer(200), 200))):
    assert fn(p, kv, m, *extra) == status, fn
    assert text in lib.ffpa_attn_last_error(), lib.ffpa_attn_last_error()
  assert lib.ffpa_attn_varlen_mla_fwd_workspace_bytes(p, kv, m) == 0


def test_the_append_must_not_write_the_lengths_it_reads(lib):
  p, kv, m, keep = _call_args(snew=1)
  keep[2].cache_seqlens = keep[0].seqused_kv
  assert lib.ffpa_attn_varlen_mla_fwd_plan(p, kv, m, (ctypes.c_int * 5)()) == 4 and b"must not be cache_seqlens" in lib.ffpa_attn_last_error()
  p, kv, m, keep = _call_args(snew=1)
  assert lib.ffpa_attn_varlen_mla_fwd_plan(p, kv, m, (ctypes.c_int * 5)()) == 0, lib.ffpa_attn_last_error()


# ----------------------------------------------------------------------------- the chunking rule
CHUNK_CASES = [(g, sq) for g in (1, 16, 64, 128) for sq in (1, 3, 4)] + [(128, 64)]


@pytest.mark.parametrize("g, sq", CHUNK_CASES)
def test_every_row_lands_in_exactly_one_chunk_of_at_most_64_rows(g, sq):
  chunks = hip.mla_row_chunks(g, sq, 64)
  assert len(chunks) == math.ceil(g * sq / 64)
  assert all(1 <= len(c) <= 64 for c in chunks)
  rows = [r for c in chunks for r in c]
  assert sorted(rows) == [(h, t) for h in range(g) for t in range(sq)] and len(set(rows)) == len(rows)
  assert rows == sorted(rows)  # head-major, in order: the chunks of a group are consecutive row tiles
  if (g, sq) == (128, 3):
    assert len(chunks) == 6 and chunks[0][-1] == (21, 0) and chunks[1][0] == (21, 1)  # a chunk boundary inside a head's tokens


@pytest.mark.parametrize("g, sq", CHUNK_CASES)
@pytest.mark.parametrize("hkv", [1, 2])
def test_the_c_plan_reports_the_same_chunks_and_grid(lib, g, sq, hkv, monkeypatch):
  monkeypatch.setenv("FFPA_HIP_FAKE_CUS", "256")
  B = 32
  p, kv, m, keep = _call_args(sq=sq, B=B, hq=g * hkv, hkv=hkv, causal=sq > 1, num_splits=1)
  plan, name = (ctypes.c_int * 5)(), ctypes.create_string_buffer(200)
  assert lib.ffpa_attn_varlen_mla_fwd_plan(p, kv, m, plan) == 0, lib.ffpa_attn_last_error()
  assert lib.ffpa_attn_varlen_mla_fwd_kernel(p, kv, m, name, 200) == 0
  row_tiles, br, bc, grid, splits = plan
  chunks = len(hip.mla_row_chunks(g, sq, 64))
  assert (br, bc, splits) == (64, 32, 1)
  assert row_tiles == chunks
  assert grid == B * hkv * chunks if g > 1 else grid == B * hkv * chunks  # one workgroup per (sequence, latent head, chunk)
  text = name.value.decode()
  assert text.startswith("ffpa_fwd_m16_mla_kernel<bf16, 576, dv=512")
  assert ("packed into rows" in text) == (g > 1) and ("chunked" in text) == (g > 1 and chunks > 1)
  # FFPA_FLAG_NO_PACK_GQA: one workgroup per query head and token tile
  p2, kv2, m2, keep2 = _call_args(sq=sq, B=B, hq=g * hkv, hkv=hkv, causal=sq > 1, num_splits=1, flags=hip.FLAG_NO_PACK_GQA)
  assert lib.ffpa_attn_varlen_mla_fwd_plan(p2, kv2, m2, plan) == 0
  assert plan[3] == B * g * hkv * math.ceil(sq / 64)


def test_the_one_reader_rule_counts_the_chunks(lib, monkeypatch):
  """The non-temporal fetch is for latent bytes with ONE reader: 64 heads x 1 token are one chunk (NT once the batch's latents outgrow the Infinity Cache), 128
  heads are two readers of every byte (never NT), whatever the size."""
  monkeypatch.setenv("FFPA_HIP_FAKE_CUS", "256")
  name = ctypes.create_string_buffer(200)
  for hq, want in ((64, True), (128, False)):
    p, kv, m, keep = _call_args(B=64, hq=hq, max_k=8192, num_splits=1)  # 64 x 8192 x 1152 B = 576 MiB of latents
    assert lib.ffpa_attn_varlen_mla_fwd_kernel(p, kv, m, name, 200) == 0
    assert (", NT>" in name.value.decode()) == want, name.value
  p, kv, m, keep = _call_args(B=8, hq=64, max_k=8192, num_splits=1)  # 72 MiB: it fits
  assert lib.ffpa_attn_varlen_mla_fwd_kernel(p, kv, m, name, 200) == 0 and ", NT>" not in name.value.decode()


def test_the_workspace_keeps_all_d_columns(lib, monkeypatch):
  monkeypatch.setenv("FFPA_HIP_FAKE_CUS", "256")
  p, kv, m, keep = _call_args(B=2, hq=128, max_k=16384)
  plan = (ctypes.c_int * 5)()
  assert lib.ffpa_attn_varlen_mla_fwd_plan(p, kv, m, plan) == 0
  ws = lib.ffpa_attn_varlen_mla_fwd_workspace_bytes(p, kv, m)
  assert plan[4] > 1 and ws == plan[4] * 128 * 2 * (576 + 1) * 4, (list(plan), ws)
