"""FP8 (OCP e4m3) latent pools in the sparse and the tree-mask latent calls — ffpa_attn_with_kvcache_mla_sparse_fp8 / ffpa_attn_with_kvcache_mla_tree_fp8 /
ffpa_attn_varlen_with_kvcache_mla_tree_fp8: what can be checked without a GPU.  The entry points and every refusal of theirs, the fake ops, the C exports, the order
of plan_call's refusals for the two new families (through ctypes, no device), the sparse span rule in the pool's bytes, and the host replay of a gathered FP8 tile
(tools/sim_lds_layout.py ``check_mla_fp8_gather_writes``)."""
import ctypes
import importlib.util
import os
import re
import subprocess

import pytest
import torch

import ffpa_attn_amd
from ffpa_attn_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALE = 192 ** -0.5
F8 = torch.float8_e4m3fn
NEW_CALLS = ("ffpa_attn_with_kvcache_mla_sparse_fp8", "ffpa_attn_with_kvcache_mla_tree_fp8", "ffpa_attn_varlen_with_kvcache_mla_tree_fp8")


@pytest.fixture(scope="module")
def lib():
  if not hip.library_available():
    from ffpa_attn_amd import build

    build.build()
  return hip.load_library()


# ----------------------------------------------------------------------------- the Python entries
def test_the_entry_points_are_exported():
  for name in NEW_CALLS:
    assert name in ffpa_attn_amd.__all__
    assert getattr(ffpa_attn_amd, name) is getattr(ffpa_attn_amd.kvcache, name)


def _sparse_args(T=3, hq=16, hkv=1, d=576, rows=256, topk=40, dtype=F8, device="cpu"):
  q = torch.zeros(T, hq, d, dtype=torch.bfloat16, device=device)
  pool = torch.zeros(rows, hkv, d, dtype=dtype, device=device)
  idx = torch.zeros(T, topk, dtype=torch.int32, device=device)
  lens = torch.zeros(T, dtype=torch.int32, device=device)
  return q, pool, idx, lens


def _sparse(q, pool, idx, lens=None, dv=512, **kw):
  kw.setdefault("softmax_scale", SCALE)
  return ffpa_attn_amd.ffpa_attn_with_kvcache_mla_sparse_fp8(q, pool, dv, idx, topk_lens=lens, **kw)


def _tree_args(B=2, sq=3, hq=16, hkv=1, d=576, page=64, pages=4, dtype=F8):
  q = torch.zeros(B, sq, hq, d, dtype=torch.bfloat16)
  pool = torch.zeros(B * pages, page, hkv, d, dtype=dtype)
  table = torch.arange(B * pages, dtype=torch.int32).view(B, pages)
  return q, pool, table


def _tree(q, pool, table, dv=512, **kw):
  kw.setdefault("cache_seqlens", 7)
  kw.setdefault("softmax_scale", SCALE)
  kw.setdefault("tree_mask", torch.ones(q.size(1), q.size(1), dtype=torch.bool))
  return ffpa_attn_amd.ffpa_attn_with_kvcache_mla_tree_fp8(q, pool, dv, block_table=table, **kw)


def _tree_varlen(q, pool, table, dv=512, **kw):
  """``q``: the uniform [B, Sq, Hq, D] batch, handed over packed."""
  B, sq = q.shape[:2]
  kw.setdefault("softmax_scale", SCALE)
  kw.setdefault("tree_mask", torch.ones(max(sq, 1), max(sq, 1), dtype=torch.bool))
  cu = torch.arange(B + 1, dtype=torch.int32) * sq
  return ffpa_attn_amd.ffpa_attn_varlen_with_kvcache_mla_tree_fp8(q.reshape(B * sq, *q.shape[2:]), pool, dv, cu, sq, torch.full((B,), 7, dtype=torch.int32), table, **kw)


TREE_CALLS = [(_tree, "ffpa_attn_with_kvcache_mla_tree_fp8"), (_tree_varlen, "ffpa_attn_varlen_with_kvcache_mla_tree_fp8")]


@pytest.mark.parametrize("dtype", [torch.float8_e4m3fnuz, torch.float8_e5m2, torch.float8_e5m2fnuz, torch.bfloat16, torch.uint8])
def test_only_ocp_e4m3_pools_are_served_and_the_message_is_the_dense_fp8_calls(dtype):
  q, pool, idx, lens = _sparse_args(dtype=dtype)
  with pytest.raises(TypeError, match=r"ffpa_attn_with_kvcache_mla_sparse_fp8 only supports fp16/bf16 q over a torch\.float8_e4m3fn kv_cache.*OCP e4m3 is the chip's FP8 format"):
    _sparse(q, pool, idx, lens)
  q, pool, table = _tree_args(dtype=dtype)
  for call, name in TREE_CALLS:
    with pytest.raises(TypeError, match=name + r" only supports fp16/bf16 q over a torch\.float8_e4m3fn kv_cache.*OCP e4m3 is the chip's FP8 format"):
      call(q, pool, table)


def test_q_and_kv_stay_16_bit():
  q, pool, idx, lens = _sparse_args()
  for bad in (q.float(), q.to(F8)):
    with pytest.raises(TypeError, match="fp16/bf16 q"):
      _sparse(bad, pool, idx, lens)
  q, pool, table = _tree_args()
  for call, name in TREE_CALLS:
    with pytest.raises(TypeError, match="fp16/bf16 q"):
      call(q.float(), pool, table)
  with pytest.raises(TypeError, match="kv must have q's dtype torch.bfloat16"):
    _tree(q, pool, table, kv=torch.zeros(2, 3, 1, 576, dtype=F8))
  with pytest.raises(TypeError, match="kv must have q's dtype torch.bfloat16"):
    _tree_varlen(q, pool, table, kv=torch.zeros(6, 1, 576, dtype=torch.float16))


def test_kv_scale_is_a_finite_positive_host_float():
  q, pool, idx, lens = _sparse_args()
  tq, tpool, table = _tree_args()
  calls = [(lambda **kw: _sparse(q, pool, idx, lens, **kw), NEW_CALLS[0])] + [(lambda c=c, **kw: c(tq, tpool, table, **kw), n) for c, n in TREE_CALLS]
  for call, name in calls:
    for bad in (torch.tensor(0.5), torch.tensor([0.5])):
      with pytest.raises(TypeError, match=name + ": kv_scale must be a host float, not a tensor.*read-back"):
        call(kv_scale=bad)
    for bad in ("0.5", None, True):
      with pytest.raises(TypeError, match=name + ": kv_scale must be a real number"):
        call(kv_scale=bad)
    for bad in (0.0, -1.0, float("inf"), float("nan"), 1e-320):
      with pytest.raises(ValueError, match=name + ": kv_scale must be finite and > 0"):
        call(kv_scale=bad)


def test_the_sparse_calls_rules_hold_under_the_new_name():
  """Every refusal of the 16-bit sparse call (tests/test_kvcache_mla_sparse.py), under the FP8 call's name: the checks are written once."""
  name = "ffpa_attn_with_kvcache_mla_sparse_fp8"
  q, pool, idx, lens = _sparse_args()
  for kw in ({}, {"softmax_scale": None}):
    with pytest.raises(TypeError, match=name + ": softmax_scale is required"):
      ffpa_attn_amd.ffpa_attn_with_kvcache_mla_sparse_fp8(q, pool, 512, idx, **kw)
  with pytest.raises(TypeError, match=name + ": softmax_scale must be a real number"):
    _sparse(q, pool, idx, lens, softmax_scale="1")
  with pytest.raises(TypeError, match=name + ": indices must be a tensor, got list"):
    _sparse(q, pool, [[0]], lens)
  with pytest.raises(NotImplementedError, match=name + " is inference only: q requires grad"):
    _sparse(q.clone().requires_grad_(True), pool, idx, lens)
  with pytest.raises(ValueError, match=name + r": q must be \[T, Hq, D\]"):
    _sparse(q[None], pool, idx, lens)
  with pytest.raises(ValueError, match=name + ": head dim of the cache .512. differs from q's .576."):
    _sparse(q, pool[..., :512], idx, lens)
  with pytest.raises(TypeError, match=name + ": head_dim_v must be an int"):
    _sparse(q, pool, idx, lens, dv=512.0)
  with pytest.raises(ValueError, match=name + r": \(D, head_dim_v\) = \(576, 500\)"):
    _sparse(q, pool, idx, lens, dv=500)
  with pytest.raises(NotImplementedError, match=name + r": \(D, head_dim_v\) = \(576, 448\) is not built"):
    _sparse(q, pool, idx, lens, dv=448)
  with pytest.raises(ValueError, match=name + ": query num_heads .16. must be a multiple of the latent num_heads .3."):
    _sparse(q, torch.zeros(256, 3, 576, dtype=F8), idx, lens)
  with pytest.raises(ValueError, match=name + ": num_splits must be a non-negative int"):
    _sparse(q, pool, idx, lens, num_splits=-1)
  with pytest.raises(ValueError, match=name + ": kv_cache must have a contiguous last dimension"):
    _sparse(q, torch.zeros(256, 1, 1152, dtype=F8)[..., ::2], idx, lens)
  with pytest.raises(NotImplementedError, match=name + ": per-head index rows"):
    _sparse(q, pool, idx[:, None], lens)
  with pytest.raises(ValueError, match=name + r": indices must be an int32 tensor \[T=3, topk\]"):
    _sparse(q, pool, idx.long(), lens)
  with pytest.raises(ValueError, match=name + ": indices needs at least one entry per token"):
    _sparse(q, pool, idx[:, :0], lens)
  with pytest.raises(ValueError, match=name + ": indices must have a contiguous last dimension"):
    _sparse(q, pool, idx[:, ::2], lens)
  with pytest.raises(ValueError, match=name + r": topk_lens must be an int32 tensor \[T=3\]"):
    _sparse(q, pool, idx, lens.long())
  with pytest.raises(ValueError, match=name + ": kv_cache must be a non-empty pool"):
    _sparse(q, pool[:0], idx, lens)
  with pytest.raises(ValueError, match=name + ": the pages of kv_cache must be evenly spaced"):
    _sparse(q, torch.zeros(4, 20, 1, 576, dtype=F8)[:, :16], idx, lens)
  with pytest.raises(NotImplementedError, match="_mla_sparse_fp8_fwd_hip"):  # (no quiet fall-back on a CPU tensor: the op has a GPU kernel or nothing)
    _sparse(q, pool, idx, lens)
  # no token: nothing is launched, the shapes stay
  q0, pool0, idx0, lens0 = _sparse_args(T=0)
  out, lse = _sparse(q0, pool0, idx0, lens0, return_softmax_lse=True)
  assert out.shape == (0, 16, 512) and out.dtype == torch.bfloat16 and lse.shape == (16, 0) and lse.dtype == torch.float32


def test_an_fp8_pools_strides_and_span_are_refused_from_sizes_and_strides():
  """The two rules ``mla_sparse_pool`` states for a pool of one byte per element, in front of any launch and without touching memory (meta tensors): row and head
  strides multiples of 16 elements; the rows of a latent head span at most 2^31 BYTES — twice the rows of a 16-bit pool."""
  name = "ffpa_attn_with_kvcache_mla_sparse_fp8"
  q, _, idx, lens = _sparse_args(device="meta")
  for shape, cut in (((256, 1, 584), 576), ((256, 2, 584), 576)):  # row stride 584 / head stride 584: multiples of 8, not of 16
    pool = torch.empty(shape, dtype=F8, device="meta")[..., :cut]
    with pytest.raises(ValueError, match=name + r": the row and head strides of an FP8 pool \(\d+, \d+\) must be multiples of 16 elements"):
      _sparse(q, pool, idx, lens)
  ok = torch.empty(256, 1, 592, dtype=F8, device="meta")[..., :576]  # (592 = 37 x 16)
  assert _sparse(q, ok, idx, lens).shape == (3, 16, 512)
  most = ((1 << 31) - 576) // 576 + 1  # the most dense 576-wide rows whose span is <= 2^31 bytes
  assert most == 3728270 and (most - 1) * 576 + 576 <= 1 << 31 < most * 576 + 576
  assert hip.mla_sparse_pool(torch.empty(most, 1, 576, dtype=F8, device="meta")) == (most, 576, 576)
  assert _sparse(q, torch.empty(most, 1, 576, dtype=F8, device="meta"), idx, lens).shape == (3, 16, 512)
  with pytest.raises(ValueError, match=name + r": the pool's rows span \d+ bytes per latent head.*2\^31"):
    _sparse(q, torch.empty(most + 1, 1, 576, dtype=F8, device="meta"), idx, lens)
  # the 16-bit pool of that many rows is out of the 16-bit call's reach: the FP8 pool holds twice the rows
  with pytest.raises(ValueError, match="ffpa_attn_with_kvcache_mla_sparse: the pool's rows span"):
    ffpa_attn_amd.ffpa_attn_with_kvcache_mla_sparse(q, torch.empty(most, 1, 576, dtype=torch.bfloat16, device="meta"), 512, idx, softmax_scale=SCALE)


def test_the_tree_calls_rules_hold_under_the_new_names():
  q, pool, table = _tree_args()
  for call, name in TREE_CALLS:
    with pytest.raises(TypeError, match=name + ": softmax_scale is required"):
      call(q, pool, table, softmax_scale=None)
    with pytest.raises(NotImplementedError, match=name + r": \(D, head_dim_v\) = \(576, 448\) is not built"):
      call(q, pool, table, dv=448)
    with pytest.raises(ValueError, match=name + ": page_size .96. must be a positive multiple of 64"):
      call(q, _tree_args(page=128)[1][:, :96], table)
    with pytest.raises(NotImplementedError, match=name + " is inference only: q requires grad"):
      call(q.clone().requires_grad_(True), pool, table)
    with pytest.raises(NotImplementedError, match=name + " is inference only: tree_mask requires grad"):
      call(q, pool, table, tree_mask=torch.ones(3, 3).requires_grad_(True))
    with pytest.raises((TypeError, ValueError), match=name):  # (the mask is checked behind _mla_check, by the 16-bit calls' _tree_words under this call's name)
      call(q, pool, table, tree_mask=torch.ones(2, 2, dtype=torch.bool))
    with pytest.raises(NotImplementedError, match="_mla_tree_fp8_fwd_hip"):  # (no quiet fall-back on a CPU tensor)
      call(q, pool, table)
  with pytest.raises(ValueError, match=r"ffpa_attn_with_kvcache_mla_tree_fp8: kv must be \[B=2, Snew, Hkv=1, D=576\]"):
    _tree(q, pool, table, kv=torch.zeros(2, 1, 2, 576, dtype=torch.bfloat16))
  with pytest.raises(ValueError, match="multiple of 64"):  # a contiguous cache of capacity 100
    ffpa_attn_amd.ffpa_attn_with_kvcache_mla_tree_fp8(q, torch.zeros(2, 100, 1, 576, dtype=F8), 512, tree_mask=torch.ones(3, 3, dtype=torch.bool), cache_seqlens=7,
                                                      softmax_scale=SCALE)
  with pytest.raises(TypeError, match="ffpa_attn_varlen_with_kvcache_mla_tree_fp8: cache_seqlens must be a tensor"):
    ffpa_attn_amd.ffpa_attn_varlen_with_kvcache_mla_tree_fp8(q.view(6, 16, 576), pool, 512, torch.tensor([0, 3, 6], dtype=torch.int32), 3, 7, table,
                                                             tree_mask=torch.ones(3, 3, dtype=torch.bool), softmax_scale=SCALE)
  # empty batches return without a launch — and without a look at the mask
  out, lse = _tree(q[:, :0], pool, table, tree_mask=None, return_softmax_lse=True)
  assert out.shape == (2, 0, 16, 512) and lse.shape == (2, 16, 0)
  out, lse = _tree_varlen(q[:, :0], pool, table, tree_mask=None, return_softmax_lse=True)
  assert out.shape == (0, 16, 512) and lse.shape == (16, 0)


@pytest.mark.parametrize("kw", [dict(causal=True), dict(kv=torch.zeros(3, 1, 576)), dict(rotary_cos=torch.zeros(256, 32)), dict(window_size=(64, 0)), dict(softcap=30.0),
                                dict(tree_mask=torch.ones(1, 1, dtype=torch.bool)), dict(alibi_slopes=torch.zeros(16)), dict(k_scale=1.0)])
def test_the_sparse_call_refuses_unserved_keywords_by_name(kw):
  q, pool, idx, lens = _sparse_args()
  with pytest.raises(NotImplementedError, match=f"ffpa_attn_with_kvcache_mla_sparse_fp8 does not support: {next(iter(kw))}"):
    _sparse(q, pool, idx, lens, **kw)


@pytest.mark.parametrize("kw", [dict(causal=True), dict(rotary_cos=torch.zeros(256, 32)), dict(window_size=(64, 0)), dict(softcap=30.0), dict(alibi_slopes=torch.zeros(16)),
                                dict(cache_batch_idx=torch.zeros(2, dtype=torch.int32)), dict(k_scale=1.0)])
def test_the_tree_calls_refuse_unserved_keywords_by_name(kw):
  q, pool, table = _tree_args()
  for call, name in TREE_CALLS:
    with pytest.raises(NotImplementedError, match=f"{name} does not support: {next(iter(kw))}"):
      call(q, pool, table, **kw)


def test_the_16_bit_calls_still_refuse_an_fp8_pool_and_point_at_the_new_calls():
  q, pool, idx, lens = _sparse_args()
  with pytest.raises(TypeError, match="ffpa_attn_with_kvcache_mla_sparse only supports fp16/bf16 q/kv_cache of one dtype"):
    ffpa_attn_amd.ffpa_attn_with_kvcache_mla_sparse(q, pool, 512, idx, topk_lens=lens, softmax_scale=SCALE)
  q, pool, table = _tree_args()
  mask = torch.ones(3, 3, dtype=torch.bool)
  with pytest.raises(TypeError, match="ffpa_attn_with_kvcache_mla_tree only supports fp16/bf16 q/kv_cache of one dtype"):
    ffpa_attn_amd.ffpa_attn_with_kvcache_mla_tree(q, pool, 512, tree_mask=mask, cache_seqlens=7, block_table=table, softmax_scale=SCALE)
  with pytest.raises(TypeError, match="ffpa_attn_varlen_with_kvcache_mla_tree only supports fp16/bf16 q/kv_cache of one dtype"):
    ffpa_attn_amd.ffpa_attn_varlen_with_kvcache_mla_tree(q.view(6, 16, 576), pool, 512, torch.tensor([0, 3, 6], dtype=torch.int32), 3, torch.full((2,), 7, dtype=torch.int32),
                                                         table, tree_mask=mask, softmax_scale=SCALE)
  assert "ffpa_attn_with_kvcache_mla_sparse_fp8" in ffpa_attn_amd.ffpa_attn_with_kvcache_mla_sparse.__doc__
  # (the tree calls' docstrings are pinned byte for byte by tests/golden/mla_front_calls.json: the module's docstring names their FP8 twins)
  for name in NEW_CALLS:
    assert name in ffpa_attn_amd.kvcache.__doc__


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_the_ops_have_fakes(dtype):
  q = torch.empty(12, 128, 576, dtype=dtype, device="meta")
  pool = torch.empty(40, 64, 1, 576, dtype=F8, device="meta")
  i32 = lambda *s: torch.empty(s, dtype=torch.int32, device="meta")
  words = torch.empty(3, 4, dtype=torch.int64, device="meta")
  o, lse = torch.ops.ffpa_attn._mla_tree_fp8_fwd_hip(q, pool, 512, 0.25, i32(4), i32(3), i32(3, 8), words, None, None, 4, 512, 0.07)
  assert o.shape == (12, 128, 512) and o.dtype == dtype and lse.shape == (128, 12) and lse.dtype == torch.float32
  o, lse = torch.ops.ffpa_attn._mla_sparse_fp8_fwd_hip(q, pool, 512, 0.25, i32(12, 300), i32(12), 0.07, 3)
  assert o.shape == (12, 128, 512) and o.dtype == dtype and lse.shape == (128, 12) and lse.dtype == torch.float32
  # ... and the public calls run on meta tensors through them
  idx, lens = i32(12, 300), i32(12)
  for ln in (None, lens):
    out, lse = ffpa_attn_amd.ffpa_attn_with_kvcache_mla_sparse_fp8(q, pool, 512, idx, topk_lens=ln, kv_scale=0.5, softmax_scale=SCALE, return_softmax_lse=True)
    assert out.shape == (12, 128, 512) and out.dtype == dtype and out.device.type == "meta" and lse.shape == (128, 12)


# ----------------------------------------------------------------------------- the C ABI
NEW_SYMBOLS = tuple("ffpa_attn_varlen_mla_tree_fp8_fwd" + s for s in ("", "_plan", "_kernel", "_workspace_bytes", "_compact_slots")) + tuple(
  "ffpa_attn_varlen_mla_sparse_fp8_fwd" + s for s in ("", "_plan", "_kernel", "_workspace_bytes"))


def test_abi_version_stays_7_and_the_symbols_are_exported_and_declared(lib, tmp_path):
  assert hip.ABI_VERSION == 7 and lib.ffpa_attn_query(0) == 7
  for name in NEW_SYMBOLS:
    assert name in hip.EXPORTS and getattr(lib, name) is not None, name
  header = open(os.path.join(ROOT, "include", "ffpa_attn.h")).read()
  declared = set(re.findall(r"^\s*(?:int|size_t|const char\*)\s+(ffpa_attn_\w+)\s*\(", header, flags=re.M))
  assert set(NEW_SYMBOLS) <= declared and declared == set(hip.EXPORTS)
  # the header compiles as C, with every new function named, and adds no struct: ffpa_mla_fp8 carries the scale
  src = tmp_path / "decl.c"
  src.write_text('#include <stdio.h>\n#include "ffpa_attn.h"\nint main(void){\nvoid* fns[] = {' + ", ".join(f"(void*){n}" for n in NEW_SYMBOLS) +
                 '};\nprintf("%d %zu %zu\\n", FFPA_ATTN_ABI_VERSION, sizeof(ffpa_mla_fp8), sizeof(fns) / sizeof(fns[0]));\nreturn 0;}\n')
  subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-Wno-pedantic", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "decl.o")], check=True)
  assert re.findall(r"typedef struct (\w+)", header).count("ffpa_mla_fp8") == 1 and ctypes.sizeof(hip.FfpaMlaFp8) == 16


_KEEP = []


def _buf():
  buf = (ctypes.c_char * 4096)()
  _KEEP.append(buf)
  return (ctypes.addressof(buf) + 15) & ~15


def _f8(kv_scale=0.5, over=None):
  f8 = hip._stamped(hip.FfpaMlaFp8)
  f8.kv_scale = kv_scale
  for k_, v_ in (over or {}).items():
    setattr(f8, k_, v_)
  return f8


# What every refusal of an ffpa_mla_fp8 looks like, first in both families.
F8_CASES = [
  (dict(no_f8=True), 1, b"mla_fp8 is NULL"),
  (dict(f8_over=dict(struct_size=8)), 10, b"ffpa_mla_fp8 ABI mismatch"),
  (dict(f8_over=dict(struct_size=0)), 10, b"ffpa_mla_fp8 ABI mismatch"),
  (dict(f8_over=dict(reserved=1)), 10, b"ffpa_mla_fp8.reserved"),
  (dict(f8_over=dict(reserved2=1.0)), 10, b"reserved2"),
  (dict(kv_scale=0.0), 4, b"ffpa_mla_fp8.kv_scale"),
  (dict(kv_scale=-0.5), 4, b"kv_scale=-0.5 must be finite and > 0"),
  (dict(kv_scale=float("inf")), 4, b"ffpa_mla_fp8.kv_scale"),
  (dict(kv_scale=float("nan")), 4, b"ffpa_mla_fp8.kv_scale"),
]


# ---- the sparse FP8 family: check_mla_fp8, check_sparse, the plan, check_mla, check_sparse_pool (span in bytes of ONE-byte elements), check_fp8_strides
def _sparse_c_args(group=16, T=4, topk=64, hkv=1, num_splits=1, flags=0, num_rows=1024, over=None, sover=None, f8_over=None, no_f8=False, kv_scale=0.5):
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
  f8 = _f8(kv_scale, f8_over)
  return (ctypes.byref(p), ctypes.byref(s), None if no_f8 else ctypes.byref(f8)), (p, s, f8)


SPARSE_BAD = dict(sover=dict(struct_size=56))  # the family's own first refusal: an ffpa_mla_fp8 error must win over it


@pytest.mark.parametrize("kw, status, text", [(dict(SPARSE_BAD, **kw), st, tx) for kw, st, tx in F8_CASES] + [
  # the sparse family's own refusals, in its order ...
  (dict(sover=dict(struct_size=56)), 10, b"ffpa_mla_sparse ABI mismatch: size 56 (want 64)"),
  (dict(sover=dict(reserved=1)), 10, b"reserved"),
  (dict(over=dict(abi_version=6)), 10, b"ffpa_varlen_fwd_params ABI mismatch"),
  (dict(over=dict(max_seqlen_q=2)), 4, b"max_seqlen_q=2"),
  (dict(sover=dict(topk=0)), 4, b"topk=0"),
  (dict(sover=dict(indices=None)), 1, b"indices must be non-NULL"),
  (dict(sover=dict(indices_stride=10)), 5, b"indices_stride=10 is smaller than topk=64"),
  (dict(over=dict(dtype=2)), 2, b"dtype"),
  (dict(sover=dict(head_dim_v=448)), 3, b"(576, 448) is not built"),
  (dict(sover=dict(kv_stride=[512, 576])), 5, b"rows must not overlap"),
  # ... each in front of the stride rule, which comes last
  (dict(sover=dict(kv_stride=[584, 576], indices_stride=10)), 5, b"indices_stride=10"),
  (dict(sover=dict(kv_stride=[584, 576], head_dim_v=448)), 3, b"(576, 448) is not built"),
  (dict(sover=dict(kv_stride=[584, 576], num_rows=1 << 23)), 4, b"the pool's rows span"),
  (dict(sover=dict(kv_stride=[584, 576])), 5, b"FP8 pool strides (row 584, head 576, page 0) must be multiples of 16 elements"),
  (dict(hkv=2, sover=dict(kv_stride=[1152, 584])), 5, b"FP8 pool strides (row 1152, head 584, page 0) must be multiples of 16 elements"),
])
def test_the_order_of_the_sparse_fp8_familys_refusals(lib, kw, status, text):
  args, keep = _sparse_c_args(**kw)
  for fn, extra in ((lib.ffpa_attn_varlen_mla_sparse_fp8_fwd, (None,)), (lib.ffpa_attn_varlen_mla_sparse_fp8_fwd_plan, ((ctypes.c_int * 5)(),)),
                    (lib.ffpa_attn_varlen_mla_sparse_fp8_fwd_kernel, (ctypes.create_string_buffer(200), 200))):
    assert fn(*args, *extra) == status, fn
    assert text in lib.ffpa_attn_last_error(), lib.ffpa_attn_last_error()
  assert lib.ffpa_attn_varlen_mla_sparse_fp8_fwd_workspace_bytes(*args) == 0


def test_the_sparse_span_is_counted_in_the_fp8_pools_bytes(lib):
  """(num_rows - 1) x row stride + head_dim <= 2^31 with ONE byte per element: the largest pool within 2^31 bytes is accepted, one row more refused — where the
  16-bit call refuses half as many rows."""
  stride = 1 << 20  # rows 1 MiB apart (a multiple of 16, below 2^24)
  rows = ((1 << 31) - 576) // stride + 1  # 2048: (rows - 1) x 2^20 + 576 < 2^31 ...
  assert rows == 2048
  plan = (ctypes.c_int * 5)()
  args, keep = _sparse_c_args(num_rows=rows, sover=dict(kv_stride=[stride, 576]))
  assert lib.ffpa_attn_varlen_mla_sparse_fp8_fwd_plan(*args, plan) == 0, lib.ffpa_attn_last_error()
  args, keep = _sparse_c_args(num_rows=rows + 1, sover=dict(kv_stride=[stride, 576]))
  assert lib.ffpa_attn_varlen_mla_sparse_fp8_fwd_plan(*args, plan) == 4
  assert b"the pool's rows span 2147484224 bytes per head" in lib.ffpa_attn_last_error() and b"* 1 + head_dim * 1" in lib.ffpa_attn_last_error()
  # dense rows: the last pool that fits and the first that does not.  (A span of EXACTLY 2^31 does not exist at head_dim 576: 2^31 - 576 = 64 x 33554423 has no
  # divisor that is a legal row stride — a multiple of 16 in [576, 2^24) —, so the boundary is tested from both sides at the nearest spans, 2^31 - 128 and 2^31 + 448.)
  assert not [st for st in range(576, 1 << 24, 16) if ((1 << 31) - 576) % st == 0]
  exact = ((1 << 31) - 576) // 576
  assert exact == 3728269 and exact * 576 + 576 == (1 << 31) - 128
  args, keep = _sparse_c_args(num_rows=exact + 1, sover=dict(kv_stride=[576, 576]))
  assert lib.ffpa_attn_varlen_mla_sparse_fp8_fwd_plan(*args, plan) == 0, lib.ffpa_attn_last_error()
  args, keep = _sparse_c_args(num_rows=exact + 2, sover=dict(kv_stride=[576, 576]))
  assert lib.ffpa_attn_varlen_mla_sparse_fp8_fwd_plan(*args, plan) == 4 and b"span 2147484096 bytes" in lib.ffpa_attn_last_error()
  # the 16-bit export on the same geometry: half the rows
  a16 = args[:2]
  keep[1].num_rows = exact // 2 + 2
  assert lib.ffpa_attn_varlen_mla_sparse_fwd_plan(*a16, plan) == 4 and b"* 2 + head_dim * 2" in lib.ffpa_attn_last_error()
  keep[1].num_rows = exact // 2 + 1
  assert lib.ffpa_attn_varlen_mla_sparse_fwd_plan(*a16, plan) == 0, lib.ffpa_attn_last_error()


@pytest.mark.parametrize("group", [16, 72, 128])
@pytest.mark.parametrize("hkv", [1, 2])
def test_the_sparse_fp8_plan_is_the_sparse_calls(lib, group, hkv, monkeypatch):
  monkeypatch.setenv("FFPA_HIP_FAKE_CUS", "256")
  for T, topk in ((1, 2048), (6, 300), (32, 2048), (5, 1)):
    for ns, flags in ((0, 0), (1, 0), (3, hip.FLAG_FORCE_SPLITS), (5, hip.FLAG_FORCE_SPLITS)):
      args, keep = _sparse_c_args(group, T, topk, hkv, ns, flags)
      got, want = (ctypes.c_int * 5)(), (ctypes.c_int * 5)()
      n8, n16 = ctypes.create_string_buffer(256), ctypes.create_string_buffer(256)
      assert lib.ffpa_attn_varlen_mla_sparse_fp8_fwd_plan(*args, got) == 0, lib.ffpa_attn_last_error()
      assert lib.ffpa_attn_varlen_mla_sparse_fwd_plan(*args[:2], want) == 0, lib.ffpa_attn_last_error()
      assert list(got) == list(want)
      assert lib.ffpa_attn_varlen_mla_sparse_fp8_fwd_workspace_bytes(*args) == lib.ffpa_attn_varlen_mla_sparse_fwd_workspace_bytes(*args[:2])
      assert lib.ffpa_attn_varlen_mla_sparse_fp8_fwd_kernel(*args, n8, 256) == 0 and lib.ffpa_attn_varlen_mla_sparse_fwd_kernel(*args[:2], n16, 256) == 0
      assert n8.value.startswith(b"ffpa_fwd_m16_mla_sparse_fp8_kernel<bf16, 576, dv=512") and b"compact" not in n8.value
      assert n8.value == n16.value.replace(b"ffpa_fwd_m16_mla_sparse_kernel", b"ffpa_fwd_m16_mla_sparse_fp8_kernel")


# ---- the tree FP8 family: check_mla_fp8, the plan under the causal flag, check_paged, check_mla, check_tree, check_fp8_strides
def _tree_c_args(d=576, dv=512, sq=4, B=32, hq=128, hkv=1, max_k=4096, causal=False, num_splits=0, flags=0, total_q=None, over=None, f8_over=None, no_f8=False,
                 row_stride=None, page_stride=None, kv_scale=0.5, tokens=None, tover=None, no_tree=False, kvover=None):
  row = row_stride if row_stride is not None else hkv * d
  p = hip._varlen_params(torch.bfloat16, B, hq, hkv, d, sq, max_k, B * sq if total_q is None else total_q, [(hq * d, d), (row, d), (row, d), (hq * dv, dv)], causal,
                         SCALE, -1.0, flags, num_splits)
  base = _buf()
  p.q = p.k = p.o = p.cu_seqlens_q = p.seqused_kv = base
  p.workspace, p.workspace_bytes = base, 0xFFFFFFFFFFFFFFFF
  for k_, v_ in (over or {}).items():
    setattr(p, k_, v_)
  pages = -(-max_k // 64)
  kv = hip._paged_kv(base, pages, pages, 64, B * pages, page_stride if page_stride is not None else 64 * row, 0)
  for k_, v_ in (kvover or {}).items():
    setattr(kv, k_, v_)
  m = hip._stamped(hip.FfpaMla)
  m.head_dim_v = dv
  tm = hip._stamped(hip.FfpaTreeMask)
  tm.bits, tm.tokens, tm.batch_stride = base, sq if tokens is None else tokens, 0
  for k_, v_ in (tover or {}).items():
    setattr(tm, k_, v_)
  f8 = _f8(kv_scale, f8_over)
  return (ctypes.byref(p), ctypes.byref(kv), ctypes.byref(m), None if no_tree else ctypes.byref(tm), None if no_f8 else ctypes.byref(f8)), (p, kv, m, tm, f8)


TREE_BAD = dict(over=dict(abi_version=6))  # the latent family's first refusal: an ffpa_mla_fp8 error must win over it


@pytest.mark.parametrize("kw, status, text", [(dict(TREE_BAD, **kw), st, tx) for kw, st, tx in F8_CASES] + [
  # the tree latent family's own refusals, in its order: params / plan, pool, latent struct, mask ...
  (dict(over=dict(abi_version=6)), 10, b"ffpa_varlen_fwd_params ABI mismatch"),
  (dict(over=dict(dtype=2)), 2, b"dtype"),
  (dict(kvover=dict(struct_size=8)), 10, b"ffpa_paged_kv"),
  (dict(dv=576), 3, b"(576, 576) is not built"),
  (dict(no_tree=True), 1, b"tree mask is NULL"),
  (dict(tover=dict(struct_size=8)), 10, b"ffpa_tree_mask ABI mismatch"),
  (dict(tover=dict(bits=None)), 1, b"tree mask bits must be non-NULL"),
  (dict(tokens=65), 4, b"tokens=65 is outside [1, 64]"),
  (dict(tokens=3), 4, b"max_seqlen_q=4 exceeds the tree mask's tokens=3"),
  (dict(tover=dict(batch_stride=2)), 5, b"batch_stride=2"),
  # ... each in front of the stride rule, which comes last
  (dict(row_stride=584, dv=576), 3, b"(576, 576) is not built"),
  (dict(row_stride=584, no_tree=True), 1, b"tree mask is NULL"),
  (dict(row_stride=584, tokens=3), 4, b"exceeds the tree mask's tokens=3"),
  (dict(row_stride=584), 5, b"FP8 pool strides (row 584, head 576, page 37376) must be multiples of 16 elements"),
  (dict(page_stride=64 * 576 + 8), 5, b"multiples of 16 elements"),
])
def test_the_order_of_the_tree_fp8_familys_refusals(lib, kw, status, text):
  args, keep = _tree_c_args(**kw)
  for fn, extra in ((lib.ffpa_attn_varlen_mla_tree_fp8_fwd, (None,)), (lib.ffpa_attn_varlen_mla_tree_fp8_fwd_plan, ((ctypes.c_int * 5)(),)),
                    (lib.ffpa_attn_varlen_mla_tree_fp8_fwd_kernel, (ctypes.create_string_buffer(200), 200)),
                    (lib.ffpa_attn_varlen_mla_tree_fp8_fwd_compact_slots, (ctypes.byref(ctypes.c_int(0)),))):
    assert fn(*args, *extra) == status, fn
    assert text in lib.ffpa_attn_last_error(), lib.ffpa_attn_last_error()
  assert lib.ffpa_attn_varlen_mla_tree_fp8_fwd_workspace_bytes(*args) == 0


TREE_PLAN_SHAPES = [dict(B=32, hq=16, sq=1, max_k=1024), dict(B=32, hq=128, sq=4, max_k=4096), dict(B=32, hq=128, sq=16, max_k=4096, causal=True),
                    dict(B=4, hq=16, sq=64, max_k=16384), dict(B=6, hq=128, sq=40, total_q=45, max_k=4096),
                    dict(B=2, hq=32, hkv=2, sq=3, max_k=300, num_splits=3, flags=hip.FLAG_FORCE_SPLITS)]


@pytest.mark.parametrize("shape", TREE_PLAN_SHAPES)
def test_the_tree_fp8_plan_is_the_tree_latent_calls(lib, shape, monkeypatch):
  """Caches far below the non-temporal rule's bytes: plan, scratch, compact grid and kernel name are the 16-bit tree latent call's — under the causal flag
  whatever the params say."""
  monkeypatch.setenv("FFPA_HIP_FAKE_CUS", "256")
  args, keep = _tree_c_args(**shape)
  a16 = args[:4]
  got, want = (ctypes.c_int * 5)(), (ctypes.c_int * 5)()
  assert lib.ffpa_attn_varlen_mla_tree_fp8_fwd_plan(*args, got) == 0, lib.ffpa_attn_last_error()
  assert lib.ffpa_attn_varlen_mla_tree_fwd_plan(*a16, want) == 0, lib.ffpa_attn_last_error()
  assert list(got) == list(want)
  assert lib.ffpa_attn_varlen_mla_tree_fp8_fwd_workspace_bytes(*args) == lib.ffpa_attn_varlen_mla_tree_fwd_workspace_bytes(*a16)
  s8, s16 = ctypes.c_int(-1), ctypes.c_int(-1)
  assert lib.ffpa_attn_varlen_mla_tree_fp8_fwd_compact_slots(*args, ctypes.byref(s8)) == 0 and lib.ffpa_attn_varlen_mla_tree_fwd_compact_slots(*a16, ctypes.byref(s16)) == 0
  assert s8.value == s16.value
  n8, n16 = ctypes.create_string_buffer(256), ctypes.create_string_buffer(256)
  assert lib.ffpa_attn_varlen_mla_tree_fp8_fwd_kernel(*args, n8, 256) == 0 and lib.ffpa_attn_varlen_mla_tree_fwd_kernel(*a16, n16, 256) == 0
  assert n8.value.startswith(b"ffpa_fwd_m16_mla_tree_fp8_kernel<bf16, 576, dv=512")
  assert n8.value == n16.value.replace(b"ffpa_fwd_m16_mla_tree_kernel", b"ffpa_fwd_m16_mla_tree_fp8_kernel")


def test_the_new_plans_price_the_cache_at_one_byte_per_element(lib, monkeypatch):
  """One reader per byte, B x keys x 576 elements: 272 MiB of bf16 is 136 MiB of e4m3 — the 16-bit twins take the NT build, the FP8 calls on the same shape do
  not; at twice the keys all do."""
  monkeypatch.setenv("FFPA_HIP_FAKE_CUS", "256")
  keys = -(-(272 << 20) // (32 * 576 * 2) // 64) * 64
  tree, sparse = {}, {}
  for mult in (1, 2):
    n8, n16 = ctypes.create_string_buffer(256), ctypes.create_string_buffer(256)
    args, keep = _tree_c_args(B=32, hq=16, sq=1, max_k=keys * mult)
    assert lib.ffpa_attn_varlen_mla_tree_fp8_fwd_kernel(*args, n8, 256) == 0 and lib.ffpa_attn_varlen_mla_tree_fwd_kernel(*args[:4], n16, 256) == 0
    tree[mult] = (b", NT>" in n8.value, b", NT>" in n16.value)
    args, keep = _sparse_c_args(16, 32, keys * mult, num_rows=1 << 20, num_splits=0)
    assert lib.ffpa_attn_varlen_mla_sparse_fp8_fwd_kernel(*args, n8, 256) == 0 and lib.ffpa_attn_varlen_mla_sparse_fwd_kernel(*args[:2], n16, 256) == 0
    sparse[mult] = (b", NT>" in n8.value, b", NT>" in n16.value)
  assert tree == {1: (False, True), 2: (True, True)}
  assert sparse == {1: (False, True), 2: (True, True)}


# ----------------------------------------------------------------------------- the LDS image of a gathered FP8 tile
def _sim():
  spec = importlib.util.spec_from_file_location("sim_lds_layout", os.path.join(ROOT, "tools", "sim_lds_layout.py"))
  sim = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(sim)
  return sim


def test_a_gathered_fp8_tile_leaves_the_16_bit_gathers_image():
  sim = _sim()
  assert sim.check_mla_fp8_gather_writes(576, quiet=True) > 100  # the seeded set: flat, row-padded and tiny pools, counts around the tile and wave boundaries, garbage tails
  # by hand: two keys of a 1024-row pool padded to 592 elements per row, the second id outside the pool (clamped), everything past the count a zero
  ids = [5, 4000, -1, (1 << 31) - 1]
  a = sim.mla_gather_image(576, ids, 2, 1024, 592, 2)
  b = sim.mla_gather_image(576, ids, 2, 1024, 592, 1)
  assert a == b
  rows = {key: {src[0] for dst, src in b.items() if dst // 1152 == key and src is not None} for key in range(32)}
  assert rows[0] == {5} and rows[1] == {1023} and all(rows[k] == set() for k in range(2, 32))
  assert sorted(src[1] for dst, src in b.items() if dst // 1152 == 0) == list(range(576))  # every column of the row, once
  # the replay is not vacuous: the image follows the ids and the count
  assert sim.mla_gather_image(576, [5, 6], 2, 1024, 576, 1) != sim.mla_gather_image(576, [6, 5], 2, 1024, 576, 1)
  assert sim.mla_gather_image(576, [5, 6], 2, 1024, 576, 1) != sim.mla_gather_image(576, [5, 6], 1, 1024, 576, 1)
  assert sim.check_mla_fp8_writes(576, quiet=True) == (1, 0)  # the ds_write_b128 pattern is the dense FP8 build's: conflict-free
