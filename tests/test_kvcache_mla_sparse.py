"""The sparse (top-k indexed) MLA latent-cache entry point without a GPU: the export, the call on meta tensors, every refusal of
``ffpa_attn_with_kvcache_mla_sparse`` (they come before any device is touched — the span refusal on meta-device pools, which allocate nothing), the two
helpers against a Python loop, ``ffpa_mla_sparse`` against its ctypes mirror and gcc, the ABI pins, the C plan (row chunks, split counts of the latent call's
plan for T one-token sequences of topk keys) and the float64 reference the GPU suite uses against a naive per-token softmax."""

import ctypes
import math
import os
import re
import subprocess

import pytest
import torch

import ffpa_attn_amd
import kvcache_mla_sparse_ref as SR
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
def test_the_entry_point_and_the_helpers_are_exported():
  for name in ("ffpa_attn_with_kvcache_mla_sparse", "compact_topk_indices", "slots_from_block_table"):
    assert name in ffpa_attn_amd.__all__
    assert getattr(ffpa_attn_amd, name) is getattr(ffpa_attn_amd.kvcache, name)


def _args(T=3, hq=16, hkv=1, d=576, rows=256, topk=40, device="cpu", dtype=torch.bfloat16):
  q = torch.zeros(T, hq, d, dtype=dtype, device=device)
  pool = torch.zeros(rows, hkv, d, dtype=dtype, device=device)
  idx = torch.zeros(T, topk, dtype=torch.int32, device=device)
  lens = torch.zeros(T, dtype=torch.int32, device=device)
  return q, pool, idx, lens


def _call(q, pool, idx, lens=None, dv=512, **kw):
  kw.setdefault("softmax_scale", SCALE)
  return ffpa_attn_amd.ffpa_attn_with_kvcache_mla_sparse(q, pool, dv, idx, topk_lens=lens, **kw)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("paged", [0, 1, 16, 64])
def test_the_call_runs_on_meta_tensors(dtype, paged):
  q, pool, idx, lens = _args(T=5, hq=128, device="meta", dtype=dtype)
  if paged:
    pool = torch.empty(7, paged, 1, 576, dtype=dtype, device="meta")
  for ln in (None, lens):
    out = _call(q, pool, idx, ln)
    assert out.shape == (5, 128, 512) and out.dtype == dtype and out.device.type == "meta"
    out, lse = _call(q, pool, idx, ln, return_softmax_lse=True, num_splits=3)
    assert out.shape == (5, 128, 512) and lse.shape == (128, 5) and lse.dtype == torch.float32
  # no token: nothing is launched, the shapes stay (CPU tensors: there is no CPU kernel to reach)
  q, pool, idx, lens = _args(T=0)
  out, lse = _call(q, pool, idx, lens, return_softmax_lse=True)
  assert out.shape == (0, 16, 512) and lse.shape == (16, 0)


def test_a_missing_scale_is_a_type_error_that_says_why():
  q, pool, idx, lens = _args()
  for kw in ({}, {"softmax_scale": None}):
    with pytest.raises(TypeError, match=r"softmax_scale is required.*1 / sqrt\(qk_nope_head_dim \+ qk_rope_head_dim\)"):
      ffpa_attn_amd.ffpa_attn_with_kvcache_mla_sparse(q, pool, 512, idx, **kw)
  with pytest.raises(TypeError, match="softmax_scale must be a real number"):
    _call(q, pool, idx, softmax_scale="0.07")


def test_argument_errors_name_the_argument():
  q, pool, idx, lens = _args()
  with pytest.raises(TypeError, match="head_dim_v must be an int"):
    _call(q, pool, idx, dv=512.0)
  with pytest.raises(ValueError, match="head_dim_v <= D"):
    _call(q, pool, idx, dv=640)
  with pytest.raises(NotImplementedError, match=r"\(576, 448\) is not built"):
    _call(q, pool, idx, dv=448)
  with pytest.raises(ValueError, match=r"q must be \[T, Hq, D\]"):
    _call(q[None], pool, idx)
  with pytest.raises(ValueError, match="kv_cache"):
    _call(q, pool[:, 0], idx)
  with pytest.raises(ValueError, match=r"head dim of the cache \(512\)"):
    _call(q, pool[..., :512], idx)
  with pytest.raises(ValueError, match=r"num_heads \(16\) must be a multiple of the latent num_heads \(3\)"):
    _call(q, _args(hkv=3)[1], idx)
  with pytest.raises(ValueError, match="num_splits"):
    _call(q, pool, idx, num_splits=-1)
  with pytest.raises(TypeError, match="fp16/bf16"):
    _call(q.float(), pool, idx)
  with pytest.raises(TypeError, match="fp16/bf16"):  # FP8 latents: a dtype error
    _call(q, pool.to(torch.float8_e4m3fn), idx)
  with pytest.raises(TypeError, match="indices must be a tensor"):
    _call(q, pool, [[0]] * 3)
  with pytest.raises(ValueError, match=r"indices must be an int32 tensor \[T=3, topk\]"):
    _call(q, pool, idx.long())
  with pytest.raises(ValueError, match=r"indices must be an int32 tensor \[T=3, topk\]"):
    _call(q, pool, idx[:2])
  with pytest.raises(ValueError, match="topk >= 1"):
    _call(q, pool, idx[:, :0])
  with pytest.raises(ValueError, match="indices must have a contiguous last dimension"):
    _call(q, pool, idx[:, ::2])
  with pytest.raises(NotImplementedError, match=r"per-head index rows \(\[T, Hkv, topk\]\) are not served"):
    _call(q, pool, idx[:, None, :])
  with pytest.raises(ValueError, match=r"topk_lens must be an int32 tensor \[T=3\]"):
    _call(q, pool, idx, lens.long())
  with pytest.raises(ValueError, match=r"topk_lens must be an int32 tensor \[T=3\]"):
    _call(q, pool, idx, lens[:2])
  with pytest.raises(TypeError, match="topk_lens must be a tensor"):
    _call(q, pool, idx, 7)
  with pytest.raises(ValueError, match="contiguous last dimension"):
    _call(q, torch.zeros(256, 1, 1152, dtype=torch.bfloat16)[..., ::2], idx)
  for i, nm in enumerate(("q", "kv_cache")):
    a = [q, pool]
    a[i] = a[i].clone().requires_grad_(True)
    with pytest.raises(NotImplementedError, match=f"inference only: {nm} requires grad"):
      _call(a[0], a[1], idx)


def test_pools_whose_pages_are_not_evenly_spaced_are_refused():
  q, _, idx, _ = _args()
  wide = torch.zeros(4, 24, 1, 576, dtype=torch.bfloat16)
  with pytest.raises(ValueError, match=r"evenly spaced.*stride\(0\) == page_size \* stride\(1\)"):
    _call(q, wide[:, :16], idx)  # (the first 16 rows of 24-row pages: slot r does not lie r rows from the base)
  halves = torch.zeros(4, 2, 16, 1, 576, dtype=torch.bfloat16)
  with pytest.raises(ValueError, match="evenly spaced"):
    _call(q, halves[:, 0], idx)
  # a padded row stride and a padded head stride are fine: the refusal past this point is the missing CPU kernel
  padded = torch.zeros(4, 16, 2, 640, dtype=torch.bfloat16)[..., :576]
  with pytest.raises(NotImplementedError, match="device 'cpu'|CPU"):
    _call(torch.zeros(3, 16, 576, dtype=torch.bfloat16), padded, idx)


def test_a_pool_beyond_the_reach_of_32_bit_offsets_is_refused_from_sizes_and_strides():
  """(num_rows - 1) x row bytes + one row <= 2^31.  The pools below live on the meta device: nothing is allocated, nothing is read."""
  q, _, idx, _ = _args(device="meta")
  meta = lambda *shape: torch.empty(shape, dtype=torch.bfloat16, device="meta")
  limit_rows = (2 ** 31 - 1152) // 1152 + 1  # the largest dense pool that fits: 1 864 135 rows
  assert hip.MLA_SPARSE_SPAN_BYTES == 2 ** 31
  fits, over = meta(limit_rows, 1, 576), meta(limit_rows + 1, 1, 576)
  assert hip.mla_sparse_pool(fits) == (limit_rows, 576, 576)
  assert _call(q, fits, idx).shape == (3, 16, 512)
  with pytest.raises(ValueError, match=rf"span {limit_rows * 1152 + 1152} bytes.*2\^31 = 2147483648"):
    hip.mla_sparse_pool(over)
  with pytest.raises(ValueError, match=r"2\^31 = 2147483648"):
    _call(q, over, idx)
  # a padded row stride reaches the limit sooner; a 4-D pool counts pages x page_size rows
  with pytest.raises(ValueError, match=r"2\^31"):
    _call(q, meta(1 << 20, 1, 1152)[..., :576], idx)
  assert _call(q, meta(1 << 19, 1, 1152)[..., :576], idx).shape == (3, 16, 512)
  with pytest.raises(ValueError, match=r"2\^31"):
    _call(q, meta(1 << 15, 64, 1, 576), idx)
  # ... and the C entry point refuses on its own (host buffers: only the plan runs)
  lib_ = hip.load_library() if hip.library_available() else None
  if lib_ is not None:
    args, keep = _plan_args(16, 4, 64, num_rows=limit_rows + 1)
    assert lib_.ffpa_attn_varlen_mla_sparse_fwd_plan(*args, (ctypes.c_int * 5)()) == 4
    assert b"2^31 = 2147483648" in lib_.ffpa_attn_last_error(), lib_.ffpa_attn_last_error()
    args, keep = _plan_args(16, 4, 64, num_rows=limit_rows)
    assert lib_.ffpa_attn_varlen_mla_sparse_fwd_plan(*args, (ctypes.c_int * 5)()) == 0, lib_.ffpa_attn_last_error()


@pytest.mark.parametrize("kw", [dict(causal=True), dict(kv=torch.zeros(3, 1, 576)), dict(rotary_cos=torch.zeros(256, 32)), dict(rotary_sin=torch.zeros(256, 32)),
                                dict(window_size=(64, 0)), dict(softcap=30.0), dict(tree_mask=torch.ones(1, 1, dtype=torch.bool)),
                                dict(alibi_slopes=torch.zeros(16)), dict(cache_batch_idx=torch.zeros(3, dtype=torch.int32)),
                                dict(cache_leftpad=torch.zeros(3, dtype=torch.int32))])
def test_unserved_keywords_raise_by_name(kw):
  q, pool, idx, lens = _args()
  with pytest.raises(NotImplementedError, match=f"does not support: {next(iter(kw))}"):
    _call(q, pool, idx, **kw)
  doc = ffpa_attn_amd.ffpa_attn_with_kvcache_mla_sparse.__doc__
  for word in ("window_size", "softcap", "tree_mask", "FP8", "topk_lens", "compact_topk_indices", "slots_from_block_table", "2^31", "causal"):
    assert word in doc


def test_the_op_has_a_fake_and_writes_nothing():
  i32 = lambda *s: torch.empty(s, dtype=torch.int32, device="meta")
  pool = torch.empty(1024, 1, 576, dtype=torch.float16, device="meta")
  o, lse = torch.ops.ffpa_attn._mla_sparse_fwd_hip(torch.empty(12, 128, 576, dtype=torch.float16, device="meta"), pool, 512, i32(12, 2048), i32(12), 0.07)
  assert o.shape == (12, 128, 512) and lse.shape == (128, 12) and lse.dtype == torch.float32
  o, lse = torch.ops.ffpa_attn._mla_sparse_fwd_hip(torch.empty(12, 128, 576, dtype=torch.float16, device="meta"), pool, 512, i32(12, 2048), None, 0.07, 4)
  assert o.shape == (12, 128, 512)
  schema = torch.ops.ffpa_attn._mla_sparse_fwd_hip.default._schema
  assert [a.name for a in schema.arguments] == ["q", "kv_cache", "head_dim_v", "indices", "topk_lens", "softmax_scale", "num_splits"]
  assert not any(a.alias_info is not None and a.alias_info.is_write for a in schema.arguments), str(schema)


# ----------------------------------------------------------------------------- the two helpers
def _compact_loop(rows):
  out, cnt = [], []
  for r in rows:
    good = [x for x in r if x >= 0]
    out.append(good + [x for x in r if x < 0])
    cnt.append(len(good))
  return out, cnt


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
def test_compact_topk_indices_against_a_loop(dtype):
  g = torch.Generator().manual_seed(3)
  rows = torch.randint(0, 1000, (9, 37), generator=g)
  rows[0] = -1                                   # an all -1 row
  rows[1, ::2] = -1                              # holes
  rows[2, :5] = -1                               # a hole in front
  rows[3, 30:] = -1                              # already compact
  rows[5, torch.randperm(37, generator=g)[:20]] = -1
  rows[6, 0] = rows[6, 1] = 7                    # duplicates keep their order and their count
  rows[7, 3] = -5                                # any negative entry is "no key"
  idx = rows.to(dtype)
  got, cnt = ffpa_attn_amd.compact_topk_indices(idx)
  want, want_cnt = _compact_loop(rows.tolist())
  assert got.dtype == dtype and cnt.dtype == torch.int32 and got.shape == idx.shape and cnt.shape == (9,)
  assert got.tolist() == want and cnt.tolist() == want_cnt
  assert cnt[0] == 0 and cnt[4] == 37  # all -1, full
  # leading batch dimensions, and idempotence
  got3, cnt3 = ffpa_attn_amd.compact_topk_indices(idx.view(3, 3, 37))
  assert got3.view(9, 37).tolist() == want and cnt3.view(9).tolist() == want_cnt
  again, cnt_again = ffpa_attn_amd.compact_topk_indices(got)
  assert again.tolist() == want and cnt_again.tolist() == want_cnt
  with pytest.raises(ValueError, match="int32 / int64"):
    ffpa_attn_amd.compact_topk_indices(idx.float())


@pytest.mark.parametrize("page", [1, 16, 64])
def test_slots_from_block_table_against_a_loop(page):
  g = torch.Generator().manual_seed(page)
  T, pps, topk = 5, 7, 23
  table = torch.randperm(T * pps, generator=g).to(torch.int32).view(T, pps)
  pos = torch.randint(0, pps * page, (T, topk), generator=g).to(torch.int32)
  pos[0] = -1
  pos[1, ::3] = -1
  pos[2] = torch.arange(topk) % (pps * page)
  got = ffpa_attn_amd.slots_from_block_table(pos, table, page)
  want = [[-1 if p < 0 else int(table[t, p // page]) * page + p % page for p in row] for t, row in enumerate(pos.tolist())]
  assert got.dtype == torch.int32 and got.tolist() == want
  assert ffpa_attn_amd.slots_from_block_table(pos.long(), table.long(), page).tolist() == want
  with pytest.raises(ValueError, match="page_size"):
    ffpa_attn_amd.slots_from_block_table(pos, table, 0)
  with pytest.raises(ValueError, match="positions must be"):
    ffpa_attn_amd.slots_from_block_table(pos, table[:2], page)


# ----------------------------------------------------------------------------- the C ABI
FIELDS = ["struct_size", "reserved", "indices", "indices_stride", "topk_lens", "kv_stride", "topk", "num_rows", "head_dim_v", "reserved2"]


def test_ctypes_mirror_of_the_struct_matches_the_c_header(tmp_path):
  fields = [f[0] for f in hip.FfpaMlaSparse._fields_]
  assert fields == FIELDS
  src = tmp_path / "layout.c"
  body = "".join(f'printf("{f} %zu\\n", offsetof(ffpa_mla_sparse, {f}));\n' for f in fields)
  src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ffpa_attn.h"\nint main(void){\n'
                 'printf("sizeof %zu\\n", sizeof(ffpa_mla_sparse));\nprintf("mla %zu\\n", sizeof(ffpa_mla));\n'
                 'printf("varlen %zu\\n", sizeof(ffpa_varlen_fwd_params));\nprintf("paged %zu\\n", sizeof(ffpa_paged_kv));\n'
                 'printf("abi %d\\n", FFPA_ATTN_ABI_VERSION);\n' + body + "return 0;}\n")
  exe = tmp_path / "layout"
  subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
  out = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
  assert int(out["sizeof"]) == ctypes.sizeof(hip.FfpaMlaSparse) == 64
  for f in fields:
    assert int(out[f]) == getattr(hip.FfpaMlaSparse, f).offset, f
  # the other structs keep their layout and the ABI version stays where it was
  assert int(out["mla"]) == ctypes.sizeof(hip.FfpaMla) == 56
  assert int(out["varlen"]) == ctypes.sizeof(hip.FfpaVarlenFwdParams) == 216 and int(out["paged"]) == ctypes.sizeof(hip.FfpaPagedKv) == 56
  assert int(out["abi"]) == 7


def test_abi_version_stays_7_and_the_symbols_are_exported_and_declared(lib):
  assert hip.ABI_VERSION == 7 and lib.ffpa_attn_query(0) == 7
  for suffix in ("", "_plan", "_kernel", "_workspace_bytes"):
    name = "ffpa_attn_varlen_mla_sparse_fwd" + suffix
    assert name in hip.EXPORTS and getattr(lib, name) is not None, name
  header = open(os.path.join(ROOT, "include", "ffpa_attn.h")).read()
  declared = set(re.findall(r"^\s*(?:int|size_t|const char\*)\s+(ffpa_attn_\w+)\s*\(", header, flags=re.M))
  assert declared == set(hip.EXPORTS)


_KEEP = []


def _buf():
  buf = (ctypes.c_char * 4096)()
  _KEEP.append(buf)
  return (ctypes.addressof(buf) + 15) & ~15


def _plan_args(group, T, topk, hkv=1, num_splits=1, flags=0, num_rows=1024, over=None, sover=None):
  """A well-formed sparse call on host buffers (only the plan and the argument checks run on it)."""
  hq, d, dv = group * hkv, 576, 512
  p, s = hip._mla_sparse_args(torch.bfloat16, T, hq, hkv, d, dv, topk, num_rows, hkv * d, d, (hq * d, d), (hq * dv, dv), SCALE, flags, num_splits)
  base = _buf()
  p.q = p.k = p.o = p.cu_seqlens_q = base
  p.workspace, p.workspace_bytes = base, 0xFFFFFFFFFFFFFFFF
  s.indices = s.topk_lens = base
  for k_, v_ in (over or {}).items():
    setattr(p, k_, v_)
  for k_, v_ in (sover or {}).items():
    if k_ == "kv_stride":
      s.kv_stride[:] = v_
    else:
      setattr(s, k_, v_)
  return (ctypes.byref(p), ctypes.byref(s)), (p, s)


def _plan(lib, args):
  plan, name = (ctypes.c_int * 5)(), ctypes.create_string_buffer(200)
  assert lib.ffpa_attn_varlen_mla_sparse_fwd_plan(*args, plan) == 0, lib.ffpa_attn_last_error()
  assert lib.ffpa_attn_varlen_mla_sparse_fwd_kernel(*args, name, 200) == 0
  return list(plan), name.value.decode()


def _latent_plan(lib, group, T, topk, hkv, num_splits, flags):
  """The latent call's plan for a batch of T one-token sequences of topk keys (tests/test_kvcache_mla_varlen.py ``_plan_args``, restated)."""
  hq, d, dv = group * hkv, 576, 512
  p = hip._varlen_params(torch.bfloat16, T, hq, hkv, d, 1, topk, T, [(hq * d, d), (hkv * d, d), (hkv * d, d), (hq * dv, dv)], False, SCALE, -1.0, flags, num_splits)
  base = _buf()
  p.q = p.k = p.o = p.cu_seqlens_q = p.seqused_kv = base
  p.workspace, p.workspace_bytes = base, 0xFFFFFFFFFFFFFFFF
  pages = -(-topk // 64)
  kv = hip._paged_kv(base, pages, pages, 64, T * pages, 64 * hkv * d, 0)
  m = hip._stamped(hip.FfpaMla)
  m.head_dim_v = dv
  plan = (ctypes.c_int * 5)()
  assert lib.ffpa_attn_varlen_mla_fwd_plan(ctypes.byref(p), ctypes.byref(kv), ctypes.byref(m), plan) == 0, lib.ffpa_attn_last_error()
  return list(plan)


@pytest.mark.parametrize("group", [16, 64, 72, 128])
@pytest.mark.parametrize("hkv", [1, 2])
def test_the_c_plan_is_the_latent_call_s_for_one_token_sequences_of_topk_keys(lib, group, hkv, monkeypatch):
  monkeypatch.setenv("FFPA_HIP_FAKE_CUS", "256")
  chunks = len(hip.mla_row_chunks(group, 1, 64))
  assert chunks == math.ceil(group / 64)
  for T, topk in ((1, 2048), (6, 300), (32, 2048), (64, 2048), (256, 64), (5, 1)):
    for ns, flags in ((0, 0), (1, 0), (3, hip.FLAG_FORCE_SPLITS), (4, 0)):
      (row_tiles, br, bc, grid, splits), name = _plan(lib, _plan_args(group, T, topk, hkv, ns, flags)[0])
      want = _latent_plan(lib, group, T, topk, hkv, ns, flags)
      assert [row_tiles, br, bc, grid, splits] == want, (T, topk, ns, flags)
      assert (br, bc) == (64, 32) and row_tiles == chunks and grid == T * hkv * chunks * splits
      assert name.startswith("ffpa_fwd_m16_mla_sparse_kernel<bf16, 576, dv=512") and "compact" not in name, name
      assert ("chunked" in name) == (chunks > 1) and ("ffpa_varlen_merge_kernel" in name) == (splits > 1)
      if flags:
        assert splits == min(ns, math.ceil(topk / 32))
  # "fill the chip": a few tokens over 2048 keys split, a full chip does not
  assert _plan(lib, _plan_args(16, 4, 2048, 1, 0)[0])[0][4] > 1
  # the workspace the launch asks for is the plan's: splits x Hq x T x (D + 1) fp32
  args, keep = _plan_args(16, 4, 2048, 1, 0)
  plan, _ = _plan(lib, args)
  assert lib.ffpa_attn_varlen_mla_sparse_fwd_workspace_bytes(*args) == plan[4] * 16 * 4 * 577 * 4


@pytest.mark.parametrize("kw, status, text", [
  (dict(sover=dict(struct_size=56)), 10, b"ffpa_mla_sparse ABI mismatch: size 56 (want 64)"),
  (dict(sover=dict(struct_size=0)), 10, b"ffpa_mla_sparse ABI mismatch"),
  (dict(sover=dict(reserved=1)), 10, b"reserved"),
  (dict(sover=dict(reserved2=1)), 10, b"reserved"),
  (dict(over=dict(struct_size=208)), 10, b"ffpa_varlen_fwd_params ABI mismatch"),
  (dict(over=dict(abi_version=6)), 10, b"ffpa_varlen_fwd_params ABI mismatch"),
  (dict(over=dict(max_seqlen_q=2)), 4, b"max_seqlen_q=2"),
  (dict(sover=dict(topk=0)), 4, b"topk=0"),
  (dict(sover=dict(num_rows=0)), 4, b"num_rows=0"),
  (dict(sover=dict(indices=None)), 1, b"indices must be non-NULL"),
  (dict(sover=dict(indices_stride=10)), 5, b"indices_stride=10 is smaller than topk=64"),
  (dict(sover=dict(head_dim_v=448)), 3, b"(576, 448) is not built"),
  (dict(sover=dict(head_dim_v=500)), 4, b"multiples of 64"),
  (dict(over=dict(dtype=2)), 2, b"dtype"),
  (dict(over=dict(batch=0)), 4, b"non-positive dimension"),
  (dict(sover=dict(kv_stride=[580, 576])), 5, b"kv stride[0]=580"),
  (dict(sover=dict(kv_stride=[512, 576])), 5, b"rows must not overlap"),
])
def test_status_codes_come_before_any_device_work(lib, kw, status, text):
  args, keep = _plan_args(16, 4, 64, **kw)
  assert lib.ffpa_attn_varlen_mla_sparse_fwd(*args, None) == status
  assert text in lib.ffpa_attn_last_error(), lib.ffpa_attn_last_error()
  assert lib.ffpa_attn_varlen_mla_sparse_fwd_plan(*args, (ctypes.c_int * 5)()) == status
  assert lib.ffpa_attn_varlen_mla_sparse_fwd_workspace_bytes(*args) == 0


def test_null_and_misaligned_arguments(lib):
  args, keep = _plan_args(16, 4, 64)
  assert lib.ffpa_attn_varlen_mla_sparse_fwd(None, args[1], None) == 1 and b"params is NULL" in lib.ffpa_attn_last_error()
  assert lib.ffpa_attn_varlen_mla_sparse_fwd(args[0], None, None) == 1 and b"mla_sparse is NULL" in lib.ffpa_attn_last_error()
  for field in ("indices", "topk_lens"):
    args, keep = _plan_args(16, 4, 64)
    setattr(keep[1], field, getattr(keep[1], field) + 2)
    assert lib.ffpa_attn_varlen_mla_sparse_fwd(*args, None) == 6 and b"4-byte aligned" in lib.ffpa_attn_last_error(), field
  # no counts is legal: every row holds topk valid entries
  args, keep = _plan_args(16, 4, 64, sover=dict(topk_lens=None))
  assert lib.ffpa_attn_varlen_mla_sparse_fwd_plan(*args, (ctypes.c_int * 5)()) == 0, lib.ffpa_attn_last_error()


# ----------------------------------------------------------------------------- the yardstick of the GPU suite
def _naive(q, pool, idx_row, n, scale, dv):
  """One token, one head at a time, in Python floats on float64 tensors: softmax(q . k_j) . v_j over the token's first n entries."""
  hq, hkv = q.size(0), pool.size(1)
  o = torch.zeros(hq, dv, dtype=torch.float64)
  lse = torch.full((hq,), float("-inf"), dtype=torch.float64)
  for h in range(hq):
    hk = h // (hq // hkv)
    s = [float((q[h].double() * pool[int(idx_row[j]), hk].double()).sum()) * scale for j in range(n)]
    if not s:
      continue
    m = max(s)
    w = [math.exp(x - m) for x in s]
    l = sum(w)
    for j in range(n):
      o[h] += (w[j] / l) * pool[int(idx_row[j]), hk, :dv].double()
    lse[h] = m + math.log(l)
  return o, lse


@pytest.mark.parametrize("case", [dict(T=3, hq=4, hkv=1, rows=40, topk=9, lens=[9, 0, 4], paged=0), dict(T=2, hq=4, hkv=2, rows=48, topk=5, lens=[1, 5], paged=16)])
def test_the_float64_reference_against_a_naive_per_token_softmax(case):
  g = torch.Generator().manual_seed(11)
  T, hq, hkv, rows, topk = case["T"], case["hq"], case["hkv"], case["rows"], case["topk"]
  q = torch.randn(T, hq, 576, generator=g).to(torch.bfloat16)
  flat = torch.randn(rows, hkv, 576, generator=g).to(torch.bfloat16)
  idx = torch.randint(0, rows, (T, topk), generator=g).to(torch.int32)
  idx[0, 1] = idx[0, 0]  # a duplicate counts twice
  for t, n in enumerate(case["lens"]):
    idx[t, n:] = -1
  pool = flat.view(rows // case["paged"], case["paged"], hkv, 576) if case["paged"] else flat
  o, lse, pmax, p2sum = SR.reference(q, pool, idx, case["lens"], SCALE, 512)
  assert o.shape == (T, 1, hq, 512) and lse.shape == (T, hq, 1) and o.dtype == torch.float64
  for t, n in enumerate(case["lens"]):
    want_o, want_lse = _naive(q[t], flat, idx[t], n, SCALE, 512)
    torch.testing.assert_close(o[t, 0], want_o, atol=1e-12, rtol=1e-12)
    torch.testing.assert_close(lse[t, :, 0], want_lse, atol=1e-12, rtol=1e-12)
    if n == 0:
      assert (o[t] == 0).all() and torch.isneginf(lse[t]).all() and (pmax[t] == 0).all()
    else:
      assert (pmax[t] > 0).all() and (pmax[t] <= 1).all() and (p2sum[t] <= 1 + 1e-12).all()
