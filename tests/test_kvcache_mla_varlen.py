"""The ragged MLA latent-cache entry point without a GPU: the export, the call on meta tensors, every refusal of ``ffpa_attn_varlen_with_kvcache_mla`` (they come
before any launch), the ops' fakes and schemas, ``ffpa_mla_append_varlen_params`` against its ctypes mirror and gcc, the ABI pins, the refusals of
``ffpa_attn_mla_append_varlen`` (before any device work), and the compact grid of packed latent rows — as a pure function and as the C plan reports it."""

import ctypes
import math
import os
import re
import subprocess

import pytest
import torch

import ffpa_attn_amd
from ffpa_attn_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALE = 192 ** -0.5

# query lengths per batch of the GPU suite (tests/test_kvcache_mla_varlen_gpu.py), with the group sizes they run at
BATCH_A = [1, 0, 3, 5, 1, 40]
BATCH_B = [1, 0, 1, 1, 1, 1, 1, 64]
BATCH_C = [1, 2, 3, 4]
BATCH_D = [70]


@pytest.fixture(scope="module")
def lib():
  if not hip.library_available():
    from ffpa_attn_amd import build

    build.build()
  return hip.load_library()


# ----------------------------------------------------------------------------- the Python entry
def test_the_entry_point_is_exported():
  from ffpa_attn_amd import ffpa_attn_varlen_with_kvcache_mla

  assert "ffpa_attn_varlen_with_kvcache_mla" in ffpa_attn_amd.__all__
  assert ffpa_attn_amd.ffpa_attn_varlen_with_kvcache_mla is ffpa_attn_varlen_with_kvcache_mla
  assert ffpa_attn_amd.kvcache.ffpa_attn_varlen_with_kvcache_mla is ffpa_attn_varlen_with_kvcache_mla


def _args(lens=(1, 0, 3), hq=16, hkv=1, d=576, page=64, pages=4, device="cpu", dtype=torch.bfloat16):
  B, T = len(lens), sum(lens)
  q = torch.zeros(T, hq, d, dtype=dtype, device=device)
  pool = torch.zeros(B * pages, page, hkv, d, dtype=dtype, device=device)
  table = torch.arange(B * pages, dtype=torch.int32, device=device).view(B, pages)
  cu = torch.tensor([0] + [sum(lens[:i + 1]) for i in range(B)], dtype=torch.int32, device=device)
  cache = torch.zeros(B, dtype=torch.int32, device=device)
  return q, pool, table, cu, cache


def _call(q, pool, table, cu, cache, dv=512, max_q=3, **kw):
  kw.setdefault("softmax_scale", SCALE)
  return ffpa_attn_amd.ffpa_attn_varlen_with_kvcache_mla(q, pool, dv, cu, max_q, cache, table, **kw)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("paged", [True, False])
def test_the_call_runs_on_meta_tensors(dtype, paged):
  lens = BATCH_A
  q, pool, table, cu, cache = _args(lens, hq=128, device="meta", dtype=dtype)
  if not paged:
    pool, table = torch.empty(len(lens), 128, 1, 576, dtype=dtype, device="meta"), None
  kv = torch.empty(sum(lens), 1, 576, dtype=dtype, device="meta")
  for new in (None, kv):
    out = _call(q, pool, table, cu, cache, max_q=40, kv=new, causal=True)
    assert out.shape == (50, 128, 512) and out.dtype == dtype and out.device.type == "meta"
    out, lse = _call(q, pool, table, cu, cache, max_q=40, kv=new, return_softmax_lse=True)
    assert out.shape == (50, 128, 512) and lse.shape == (128, 50) and lse.dtype == torch.float32
  # no token: nothing is launched, the shapes stay
  out, lse = _call(q[:0], pool, table, cu, cache, max_q=0, return_softmax_lse=True)
  assert out.shape == (0, 128, 512) and lse.shape == (128, 0)


def test_a_missing_scale_is_a_type_error_that_says_why():
  a = _args()
  for kw in ({}, {"softmax_scale": None}):
    with pytest.raises(TypeError, match=r"softmax_scale is required.*1 / sqrt\(qk_nope_head_dim \+ qk_rope_head_dim\)"):
      ffpa_attn_amd.ffpa_attn_varlen_with_kvcache_mla(a[0], a[1], 512, a[3], 3, a[4], a[2], **kw)
  with pytest.raises(TypeError, match="softmax_scale must be a real number"):
    _call(*a, softmax_scale="0.07")


def test_argument_errors_name_the_argument():
  q, pool, table, cu, cache = _args()
  with pytest.raises(TypeError, match="head_dim_v must be an int"):
    _call(q, pool, table, cu, cache, dv=512.0)
  with pytest.raises(ValueError, match="head_dim_v <= D"):
    _call(q, pool, table, cu, cache, dv=640)
  with pytest.raises(NotImplementedError, match=r"\(576, 448\) is not built"):
    _call(q, pool, table, cu, cache, dv=448)
  with pytest.raises(ValueError, match="q must be packed"):
    _call(q[None], pool, table, cu, cache)
  with pytest.raises(TypeError, match="cu_seqlens_q must be int32"):
    _call(q, pool, table, cu.long(), cache)
  with pytest.raises(ValueError, match="cu_seqlens_q must be a 1-D int32 tensor"):
    _call(q, pool, table, cu[:1], cache)
  with pytest.raises(TypeError, match="cu_seqlens_q must be a tensor"):
    _call(q, pool, table, [0, 1, 1, 4], cache)
  with pytest.raises(ValueError, match="max_seqlen_q must be a host int"):
    _call(q, pool, table, cu, cache, max_q=0)
  with pytest.raises(ValueError, match="max_seqlen_q must be a host int"):
    _call(q, pool, table, cu, cache, max_q=torch.tensor(3))
  with pytest.raises(TypeError, match="cache_seqlens must be int32"):
    _call(q, pool, table, cu, cache.long())
  with pytest.raises(ValueError, match=r"cache_seqlens must be an int32 tensor \[batch=3\]"):
    _call(q, pool, table, cu, cache[:2])
  with pytest.raises(TypeError, match="cache_seqlens must be a tensor"):
    _call(q, pool, table, cu, 7)
  with pytest.raises(ValueError, match=r"block_table must be an int32 tensor \[batch=3, pages_per_seq\]"):
    _call(q, pool, table[:2], cu, cache)
  with pytest.raises(ValueError, match="page_size .96. must be a positive multiple of 64"):
    _call(q, _args(page=128)[1][:, :96], table, cu, cache)
  with pytest.raises(ValueError, match=r"capacity \(100\) must be a positive multiple of 64"):
    _call(q, torch.zeros(3, 100, 1, 576, dtype=torch.bfloat16), None, cu, cache)
  with pytest.raises(ValueError, match="must have cu_seqlens_q's batch"):
    _call(q, torch.zeros(2, 128, 1, 576, dtype=torch.bfloat16), None, cu, cache)
  with pytest.raises(ValueError, match=r"num_heads \(16\) must be a multiple of the latent num_heads \(3\)"):
    _call(q, _args(hkv=3)[1], table, cu, cache)
  with pytest.raises(ValueError, match="num_splits"):
    _call(q, pool, table, cu, cache, num_splits=-1)
  with pytest.raises(TypeError, match="fp16/bf16"):
    _call(q.float(), pool, table, cu, cache)
  with pytest.raises(ValueError, match=r"kv must be \[T=4, Hkv=1, D=576\]"):
    _call(q, pool, table, cu, cache, kv=torch.zeros(3, 1, 576, dtype=torch.bfloat16))
  with pytest.raises(TypeError, match="kv must have the cache's dtype"):
    _call(q, pool, table, cu, cache, kv=torch.zeros(4, 1, 576, dtype=torch.float16))
  for i in range(3):
    args = [q, pool, torch.zeros(4, 1, 576, dtype=torch.bfloat16)]
    args[i] = args[i].clone().requires_grad_(True)
    with pytest.raises(NotImplementedError, match=f"inference only: {('q', 'kv_cache', 'kv')[i]} requires grad"):
      _call(args[0], args[1], table, cu, cache, kv=args[2])


@pytest.mark.parametrize("kw", [dict(rotary_cos=torch.zeros(256, 32)), dict(rotary_sin=torch.zeros(256, 32)), dict(positions=torch.zeros(4, dtype=torch.int32)),
                                dict(window_size=(64, 0)), dict(softcap=30.0), dict(tree_mask=torch.ones(1, 1, dtype=torch.bool)),
                                dict(alibi_slopes=torch.zeros(16)), dict(cache_batch_idx=torch.zeros(3, dtype=torch.int32))])
def test_unserved_keywords_raise_by_name(kw):
  with pytest.raises(NotImplementedError, match=f"does not support: {next(iter(kw))}"):
    _call(*_args(), **kw)
  doc = ffpa_attn_amd.ffpa_attn_varlen_with_kvcache_mla.__doc__
  for word in ("window_size", "softcap", "tree_mask", "rotary_cos", "positions", "FP8", "max_seqlen_q", "cache_seqlens"):
    assert word in doc


def test_the_uniform_call_still_refuses_cu_seqlens_q_and_points_here():
  q = torch.zeros(2, 1, 16, 576, dtype=torch.bfloat16)
  pool = torch.zeros(8, 64, 1, 576, dtype=torch.bfloat16)
  with pytest.raises(NotImplementedError, match="does not support: cu_seqlens_q.*ffpa_attn_varlen_with_kvcache_mla"):
    ffpa_attn_amd.ffpa_attn_with_kvcache_mla(q, pool, 512, cache_seqlens=7, block_table=torch.arange(8, dtype=torch.int32).view(2, 4), softmax_scale=SCALE,
                                             cu_seqlens_q=torch.zeros(3, dtype=torch.int32))
  assert "ffpa_attn_varlen_with_kvcache_mla" in ffpa_attn_amd.ffpa_attn_with_kvcache_mla.__doc__


def test_the_ops_have_fakes_and_the_append_schema_marks_the_cache_written():
  i32 = lambda *s: torch.empty(s, dtype=torch.int32, device="meta")
  pool = torch.empty(40, 64, 1, 576, dtype=torch.float16, device="meta")
  used = torch.ops.ffpa_attn._mla_append_varlen_hip(pool, torch.empty(12, 1, 576, dtype=torch.float16, device="meta"), i32(7), i32(6), i32(6, 5))
  assert used.shape == (6,) and used.dtype == torch.int32
  schema = torch.ops.ffpa_attn._mla_append_varlen_hip.default._schema
  written = [a.name for a in schema.arguments if a.alias_info is not None and a.alias_info.is_write]
  assert written == ["kv_cache"], str(schema)
  assert [a.name for a in schema.arguments] == ["kv_cache", "kv_new", "cu_seqlens_q", "cache_seqlens", "block_table"]
  o, lse = torch.ops.ffpa_attn._mla_fwd_hip(torch.empty(12, 128, 576, dtype=torch.float16, device="meta"), pool, 512, i32(7), used, i32(6, 5), None, None, 4, 320,
                                            0.07, 1)
  assert o.shape == (12, 128, 512) and lse.shape == (128, 12)


# ----------------------------------------------------------------------------- the C ABI
FIELDS = ["struct_size", "reserved", "kv_new", "kv_cache", "cu_seqlens_q", "cache_seqlens", "seqused", "kv_new_stride", "kv_cache_stride", "batch", "total_q",
          "heads_kv", "head_dim", "dtype", "reserved2"]


def test_ctypes_mirror_of_the_append_params_matches_the_c_header(tmp_path):
  fields = [f[0] for f in hip.FfpaMlaAppendVarlenParams._fields_]
  assert fields == FIELDS
  src = tmp_path / "layout.c"
  body = "".join(f'printf("{f} %zu\\n", offsetof(ffpa_mla_append_varlen_params, {f}));\n' for f in fields)
  src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ffpa_attn.h"\nint main(void){\n'
                 'printf("sizeof %zu\\n", sizeof(ffpa_mla_append_varlen_params));\nprintf("mla %zu\\n", sizeof(ffpa_mla));\n'
                 'printf("varlen %zu\\n", sizeof(ffpa_varlen_fwd_params));\nprintf("paged %zu\\n", sizeof(ffpa_paged_kv));\n'
                 'printf("abi %d\\n", FFPA_ATTN_ABI_VERSION);\n' + body + "return 0;}\n")
  exe = tmp_path / "layout"
  subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
  out = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
  assert int(out["sizeof"]) == ctypes.sizeof(hip.FfpaMlaAppendVarlenParams) == 104
  for f in fields:
    assert int(out[f]) == getattr(hip.FfpaMlaAppendVarlenParams, f).offset, f
  # the forward call's structs keep their layout and the ABI version stays where it was
  assert int(out["mla"]) == ctypes.sizeof(hip.FfpaMla) == 56
  assert int(out["varlen"]) == ctypes.sizeof(hip.FfpaVarlenFwdParams) == 216 and int(out["paged"]) == ctypes.sizeof(hip.FfpaPagedKv) == 56
  assert int(out["abi"]) == 7


def test_abi_version_stays_7_and_the_symbols_are_exported_and_declared(lib):
  assert hip.ABI_VERSION == 7 and lib.ffpa_attn_query(0) == 7
  for name in ("ffpa_attn_mla_append_varlen", "ffpa_attn_varlen_mla_fwd_compact_slots"):
    assert name in hip.EXPORTS and getattr(lib, name) is not None, name
  header = open(os.path.join(ROOT, "include", "ffpa_attn.h")).read()
  declared = set(re.findall(r"^\s*(?:int|size_t|const char\*)\s+(ffpa_attn_\w+)\s*\(", header, flags=re.M))
  assert declared == set(hip.EXPORTS)
  assert "ragged positions" not in header  # (the latent-cache call's not-served list)


_KEEP = []


def _buf():
  buf = (ctypes.c_char * 4096)()
  _KEEP.append(buf)
  return (ctypes.addressof(buf) + 15) & ~15


def _append_args(over=None, kv_over=None, no_kv=False, total_q=5, page=64):
  """A well-formed ragged latent append on host buffers (only the argument checks run on it) -> the ctypes arguments (p, kv | None) + their owners."""
  base = _buf()
  p = hip._stamped(hip.FfpaMlaAppendVarlenParams)
  p.kv_new, p.kv_cache, p.cu_seqlens_q, p.cache_seqlens, p.seqused = base, base + 1024, base + 2048, base + 2112, base + 2176
  p.kv_new_stride[:] = [576, 576]
  p.kv_cache_stride[:] = [576, 576]
  p.batch, p.total_q, p.heads_kv, p.head_dim, p.dtype = 4, total_q, 1, 576, 0
  for k_, v_ in (over or {}).items():
    if k_.endswith("_stride"):
      getattr(p, k_)[:] = v_
    else:
      setattr(p, k_, v_)
  kv = hip._paged_kv(base + 3072, 4, 4, page, 16, page * 576, 0)
  for k_, v_ in (kv_over or {}).items():
    setattr(kv, k_, v_)
  return ctypes.byref(p), (None if no_kv else ctypes.byref(kv)), (p, kv)


@pytest.mark.parametrize("kw, status, text", [
  (dict(over=dict(struct_size=96)), 10, b"ffpa_mla_append_varlen_params ABI mismatch"),
  (dict(over=dict(struct_size=0)), 10, b"ffpa_mla_append_varlen_params ABI mismatch"),
  (dict(over=dict(reserved=1)), 10, b"reserved"),
  (dict(over=dict(reserved2=1)), 10, b"reserved"),
  (dict(over=dict(dtype=2)), 2, b"dtype"),
  (dict(over=dict(batch=0)), 4, b"non-positive dimension"),
  (dict(over=dict(heads_kv=0)), 4, b"non-positive dimension"),
  (dict(over=dict(head_dim=572)), 3, b"headdim not support"),
  (dict(over=dict(head_dim=0)), 3, b"headdim not support"),
  (dict(over=dict(total_q=-1)), 4, b"total_q"),
  (dict(no_kv=True), 1, b"paged kv is NULL"),
  (dict(kv_over=dict(struct_size=48)), 10, b"ffpa_paged_kv ABI mismatch"),
  (dict(kv_over=dict(block_table=None)), 1, b"block_table"),
  (dict(page=96), 4, b"page_size=96 is not a positive multiple of 64"),
  (dict(page=32), 4, b"page_size=32 is not a positive multiple of 64"),
  (dict(over=dict(kv_cache=None)), 1, b"kv_cache / cu_seqlens_q / cache_seqlens / seqused must be non-NULL"),
  (dict(over=dict(cu_seqlens_q=None)), 1, b"must be non-NULL"),
  (dict(over=dict(cache_seqlens=None)), 1, b"must be non-NULL"),
  (dict(over=dict(seqused=None)), 1, b"must be non-NULL"),
  (dict(over=dict(kv_new=None)), 1, b"kv_new must be non-NULL when total_q > 0"),
  (dict(over=dict(kv_new_stride=[580, 576])), 5, b"kv_new stride[0]=580"),
  (dict(over=dict(kv_cache_stride=[576, -8])), 5, b"kv_cache stride[1]=-8"),
])
def test_status_codes_of_the_append_come_before_any_device_work(lib, kw, status, text):
  p, kv, keep = _append_args(**kw)
  assert lib.ffpa_attn_mla_append_varlen(p, kv, None) == status
  assert text in lib.ffpa_attn_last_error(), lib.ffpa_attn_last_error()


def test_append_refusals_that_need_two_pointers(lib):
  assert lib.ffpa_attn_mla_append_varlen(None, None, None) == 1 and b"params is NULL" in lib.ffpa_attn_last_error()
  p, kv, keep = _append_args()
  keep[0].seqused = keep[0].cache_seqlens
  assert lib.ffpa_attn_mla_append_varlen(p, kv, None) == 4 and b"seqused must not be cache_seqlens" in lib.ffpa_attn_last_error()
  for field, text in (("kv_new", b"16-byte aligned"), ("kv_cache", b"16-byte aligned"), ("cu_seqlens_q", b"4-byte aligned"), ("seqused", b"4-byte aligned")):
    p, kv, keep = _append_args()
    setattr(keep[0], field, getattr(keep[0], field) + 2)
    assert lib.ffpa_attn_mla_append_varlen(p, kv, None) == 6 and text in lib.ffpa_attn_last_error(), field


# ----------------------------------------------------------------------------- the compact grid of packed rows
def _plan_args(group, lens, hkv=1, max_k=512, causal=True, num_splits=1, flags=0, total_q=None):
  """A well-formed ragged latent-cache call on host buffers (only the plan runs on it)."""
  B, hq, d, dv = len(lens), group * hkv, 576, 512
  p = hip._varlen_params(torch.bfloat16, B, hq, hkv, d, max(lens), max_k, sum(lens) if total_q is None else total_q,
                         [(hq * d, d), (hkv * d, d), (hkv * d, d), (hq * dv, dv)], causal, SCALE, -1.0, flags, num_splits)
  base = _buf()
  p.q = p.k = p.o = p.cu_seqlens_q = p.seqused_kv = base
  p.workspace, p.workspace_bytes = base, 0xFFFFFFFFFFFFFFFF
  pages = -(-max_k // 64)
  kv = hip._paged_kv(base, pages, pages, 64, B * pages, 64 * hkv * d, 0)
  m = hip._stamped(hip.FfpaMla)
  m.head_dim_v = dv
  return (ctypes.byref(p), ctypes.byref(kv), ctypes.byref(m)), (p, kv, m)


def _plan(lib, args):
  plan, name, slots = (ctypes.c_int * 5)(), ctypes.create_string_buffer(200), ctypes.c_int(-1)
  assert lib.ffpa_attn_varlen_mla_fwd_plan(*args, plan) == 0, lib.ffpa_attn_last_error()
  assert lib.ffpa_attn_varlen_mla_fwd_kernel(*args, name, 200) == 0
  assert lib.ffpa_attn_varlen_mla_fwd_compact_slots(*args, ctypes.byref(slots)) == 0
  return list(plan), name.value.decode(), slots.value


MTP = [1 + i % 4 for i in range(32)]
PLAN_TABLE = [
  (128, BATCH_A), (16, BATCH_B), (16, BATCH_C), (128, BATCH_C), (1, BATCH_D),   # the GPU suite's batches
  (16, BATCH_A), (64, BATCH_A), (128, BATCH_B), (2, BATCH_B), (4, BATCH_B),
  (16, MTP), (128, MTP),                                                        # speculative verification: 1 ... 4 tokens
  (16, [1] * 63 + [64]), (128, [1] * 63 + [64]), (16, [1] * 63 + [512]), (128, [1] * 63 + [512]),  # decodes + one chunk
  (128, [1, 1, 1, 2]), (128, [1, 1, 1, 1, 1, 1, 1, 8]), (128, [0, 0, 0, 0, 0, 0, 0, 4]), (16, [0, 5, 0]), (16, [4] * 12 + [17] * 4),
  (128, [1] * 12 + [4]), (128, [1] * 20 + [16]), (128, [1] * 3 + [16]),
  (128, [1] * 7 + [10]), (128, [1] * 7 + [11]),                                  # either side of the threshold: 4 x 42 > 8 x 20, 4 x 44 <= 8 x 22
]


def test_the_issue_s_batches_take_the_grids_it_names():
  assert hip.mla_compact_slots(128, BATCH_A) == 106 and len(BATCH_A) * math.ceil(128 * 40 / 64) == 480
  assert hip.mla_compact_slots(16, BATCH_B) == 26 and len(BATCH_B) * math.ceil(16 * 64 / 64) == 128
  assert hip.mla_compact_slots(16, BATCH_C) == 0 and hip.mla_compact_slots(128, BATCH_C) == 0 and hip.mla_compact_slots(1, BATCH_D) == 0
  # workgroups that find rows: 100 of the 480, 1 150 of the 65 536 of a 512-token chunk among 63 decodes
  assert sum(len(c) for c in hip.mla_ragged_row_chunks(128, BATCH_A)[0]) == 100
  assert sum(len(c) for c in hip.mla_ragged_row_chunks(128, [1] * 63 + [512])[0]) == 1150 and 64 * math.ceil(128 * 512 / 64) == 65536


@pytest.mark.parametrize("group, lens", PLAN_TABLE)
@pytest.mark.parametrize("hkv", [1, 2])
def test_the_c_plan_takes_the_compact_grid_the_pure_rule_takes(lib, group, lens, hkv, monkeypatch):
  monkeypatch.setenv("FFPA_HIP_FAKE_CUS", "256")
  args, keep = _plan_args(group, lens, hkv)
  (row_tiles, br, bc, grid, splits), name, slots = _plan(lib, args)
  want = hip.mla_compact_slots(group, lens)
  nqt = math.ceil(group * max(lens) / 64)
  assert (br, bc, splits) == (64, 32, 1) and row_tiles == nqt
  assert slots == want, (slots, want)
  assert ("compact" in name) == (want > 0), name
  if group > 1:
    assert grid == (want if want else len(lens) * nqt) * hkv
    assert ("packed into rows" in name) and ("chunked" in name) == (nqt > 1)
  # FFPA_FLAG_NO_COMPACT_GRID: the full grid, whatever the rule says
  args2, keep2 = _plan_args(group, lens, hkv, flags=hip.FLAG_NO_COMPACT_GRID)
  plan2, name2, slots2 = _plan(lib, args2)
  assert slots2 == 0 and "compact" not in name2 and plan2[3] == len(lens) * nqt * hkv * (1 if group > 1 else group)
  # the split rule runs on the grid that is launched: with forced ranges the workgroups are grid x ranges
  args3, keep3 = _plan_args(group, lens, hkv, num_splits=3, flags=hip.FLAG_FORCE_SPLITS)
  plan3, name3, slots3 = _plan(lib, args3)
  assert slots3 == want and plan3[4] == 3 and plan3[3] == 3 * grid


def test_a_call_that_does_not_say_its_rows_keeps_the_full_grid(lib, monkeypatch):
  monkeypatch.setenv("FFPA_HIP_FAKE_CUS", "256")
  args, keep = _plan_args(128, BATCH_A, total_q=0)
  plan, name, slots = _plan(lib, args)
  assert slots == 0 and plan[3] == 480


@pytest.mark.parametrize("group", [1, 16, 64, 128])
@pytest.mark.parametrize("sq", [1, 3, 4, 64])
def test_uniform_plans_are_unchanged(lib, group, sq, monkeypatch):
  """A uniform batch never meets the three-quarter test: slots = ceil(group x B x Sq / 64) + B > B x ceil(group x Sq / 64) / 4."""
  monkeypatch.setenv("FFPA_HIP_FAKE_CUS", "256")
  for B in (1, 2, 32, 64):
    assert hip.mla_compact_slots(group, [sq] * B) == 0
    for ns in (0, 1):
      args, keep = _plan_args(group, [sq] * B, max_k=4096, causal=sq > 1, num_splits=ns)
      plan, name, slots = _plan(lib, args)
      args2, keep2 = _plan_args(group, [sq] * B, max_k=4096, causal=sq > 1, num_splits=ns, flags=hip.FLAG_NO_COMPACT_GRID)
      plan2, name2, _ = _plan(lib, args2)
      chunks = len(hip.mla_row_chunks(group, sq, 64))
      assert slots == 0 and "compact" not in name and plan == plan2 and name == name2
      assert plan[0] == chunks and plan[3] == B * chunks * plan[4]


@pytest.mark.parametrize("group, lens", PLAN_TABLE)
def test_every_packed_row_lands_in_exactly_one_chunk_of_at_most_64_rows(group, lens):
  chunks, slots = hip.mla_ragged_row_chunks(group, lens, 64)
  assert len(chunks) == len(lens)
  for n, seq in zip(lens, chunks):
    assert len(seq) == math.ceil(group * n / 64)
    assert all(1 <= len(c) <= 64 for c in seq)
    rows = [r for c in seq for r in c]
    assert rows == [(h, t) for h in range(group) for t in range(n)]  # head-major, in order, every row once
  assert sum(len(seq) for seq in chunks) <= slots == math.ceil(group * sum(lens) / 64) + len(lens)
