"""The tree-mask latent-cache entry points without a GPU: the exports, the calls on meta tensors, every refusal of ``ffpa_attn_with_kvcache_mla_tree`` and
``ffpa_attn_varlen_with_kvcache_mla_tree`` (they come before any launch), the op's fake and schema, the two plain latent calls still refusing ``tree_mask``, and —
where the library is built — the C plan against ``ffpa_attn_varlen_mla_fwd``'s under the causal flag, the kernel-name query, the refusals of a bad
``ffpa_tree_mask`` and the new kernels' code-object metadata (no scratch, no spills)."""

import ctypes
import glob
import gzip
import os
import re

import pytest
import torch

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


def test_the_entry_points_are_exported():
  for name in ("ffpa_attn_with_kvcache_mla_tree", "ffpa_attn_varlen_with_kvcache_mla_tree"):
    assert name in ffpa_attn_amd.__all__
    assert getattr(ffpa_attn_amd, name) is getattr(ffpa_attn_amd.kvcache, name)
  assert callable(hip.mla_tree_forward)


# ----------------------------------------------------------------------------- the uniform call
def _uni(B=2, sq=3, hq=16, hkv=1, d=576, page=64, pages=4, device="cpu", dtype=torch.bfloat16):
  q = torch.zeros(B, sq, hq, d, dtype=dtype, device=device)
  pool = torch.zeros(B * pages, page, hkv, d, dtype=dtype, device=device)
  table = torch.arange(B * pages, dtype=torch.int32, device=device).view(B, pages)
  mask = torch.ones(sq, sq, dtype=torch.bool, device=device).tril()
  return q, pool, table, mask


def _call(q, pool, table, mask, dv=512, lens=7, **kw):
  kw.setdefault("softmax_scale", SCALE)
  return ffpa_attn_amd.ffpa_attn_with_kvcache_mla_tree(q, pool, dv, tree_mask=mask, cache_seqlens=lens, block_table=table, **kw)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("paged", [True, False])
def test_the_uniform_call_runs_on_meta_tensors(dtype, paged):
  q, pool, table, mask = _uni(B=4, sq=5, hq=128, device="meta", dtype=dtype)
  if not paged:
    pool, table = torch.empty(4, 128, 1, 576, dtype=dtype, device="meta"), None
  kv = torch.empty(4, 5, 1, 576, dtype=dtype, device="meta")
  lens = torch.empty(4, dtype=torch.int32, device="meta")
  masks = (mask, mask[None].expand(4, 5, 5), torch.empty(1, 5, dtype=torch.int64, device="meta"), torch.empty(4, 64, dtype=torch.int64, device="meta"),
           torch.empty(64, 64, dtype=torch.bool, device="meta"))
  for m in masks:
    for new in (None, kv):
      out = _call(q, pool, table, m, lens=lens, kv=new)
      assert out.shape == (4, 5, 128, 512) and out.dtype == dtype and out.device.type == "meta"
      out, lse = _call(q, pool, table, m, lens=lens, kv=new, return_softmax_lse=True, num_splits=3)
      assert out.shape == (4, 5, 128, 512) and lse.shape == (4, 128, 5) and lse.dtype == torch.float32


def test_a_missing_scale_is_a_type_error_that_says_why():
  q, pool, table, mask = _uni()
  for kw in ({}, {"softmax_scale": None}):
    with pytest.raises(TypeError, match=r"ffpa_attn_with_kvcache_mla_tree: softmax_scale is required.*1 / sqrt\(qk_nope_head_dim \+ qk_rope_head_dim\)"):
      ffpa_attn_amd.ffpa_attn_with_kvcache_mla_tree(q, pool, 512, tree_mask=mask, cache_seqlens=7, block_table=table, **kw)
  with pytest.raises(TypeError, match="softmax_scale must be a real number"):
    _call(q, pool, table, mask, softmax_scale="0.07")
  with pytest.raises(TypeError):  # (tree_mask is a required keyword)
    ffpa_attn_amd.ffpa_attn_with_kvcache_mla_tree(q, pool, 512, cache_seqlens=7, block_table=table, softmax_scale=SCALE)


def test_uniform_argument_errors_name_the_argument():
  q, pool, table, mask = _uni()
  with pytest.raises(ValueError, match="head_dim_v <= D"):
    _call(q, pool, table, mask, dv=640)
  with pytest.raises(NotImplementedError, match=r"ffpa_attn_with_kvcache_mla_tree: \(D, head_dim_v\) = \(576, 448\) is not built"):
    _call(q, pool, table, mask, dv=448)
  q5, pool5, _, _ = _uni(d=512)
  with pytest.raises(NotImplementedError, match=r"\(512, 512\) is not built"):
    _call(q5, pool5, table, mask)
  with pytest.raises(ValueError, match=r"capacity \(100\) must be a positive multiple of 64"):
    _call(q, torch.zeros(2, 100, 1, 576, dtype=torch.bfloat16), None, mask)
  with pytest.raises(ValueError, match="num_splits"):
    _call(q, pool, table, mask, num_splits=-1)
  with pytest.raises(TypeError, match="fp16/bf16"):
    _call(q.float(), pool, table, mask)
  with pytest.raises(TypeError, match="fp16/bf16"):  # (FP8 latents: a dtype error)
    _call(q, pool.to(torch.float8_e4m3fn), table, mask)
  # the mask: W outside [Sq, 64], a batch that is neither 1 nor B, a wrong dtype / rank / device
  for bad in (torch.ones(2, 2, dtype=torch.bool), torch.ones(65, 65, dtype=torch.bool), torch.ones(1, 2, dtype=torch.int64), torch.ones(2, 65, dtype=torch.int64),
              torch.ones(3, dtype=torch.int64), torch.ones(2, 3, 3, dtype=torch.int64)):
    with pytest.raises(ValueError, match=r"ffpa_attn_with_kvcache_mla_tree: tree_mask must be bool \[W, W\].*3 <= W <= 64"):
      _call(q, pool, table, bad)
  for bad in (torch.ones(3, 3, 3, dtype=torch.bool), torch.ones(3, 5, dtype=torch.int64), torch.ones(3, 4, dtype=torch.bool)):
    with pytest.raises(ValueError, match=r"ffpa_attn_with_kvcache_mla_tree: .*B=2"):
      _call(q, pool, table, bad)
  with pytest.raises(TypeError, match="tree_mask must be a torch.bool mask or int64 packed words"):
    _call(q, pool, table, mask.to(torch.int32))
  with pytest.raises(TypeError, match="tree_mask must be a tensor"):
    _call(q, pool, table, [[True]])
  with pytest.raises(ValueError, match="tree_mask must be on q's device"):
    _call(q, pool, table, mask.to("meta"))
  q65 = torch.zeros(2, 65, 16, 576, dtype=torch.bfloat16)
  with pytest.raises(ValueError, match="1 <= Sq <= 64"):
    _call(q65, pool, table, torch.ones(64, 64, dtype=torch.bool))
  kv = torch.zeros(2, 3, 1, 576, dtype=torch.bfloat16)
  for i in range(3):
    args = [q, pool, kv]
    args[i] = args[i].clone().requires_grad_(True)
    with pytest.raises(NotImplementedError, match=f"ffpa_attn_with_kvcache_mla_tree is inference only: {('q', 'kv_cache', 'kv')[i]} requires grad"):
      _call(args[0], args[1], table, mask, kv=args[2])
  with pytest.raises(NotImplementedError, match="inference only: tree_mask requires grad"):
    _call(q, pool, table, _Grad(mask))


class _Grad(torch.Tensor):
  """A bool mask that claims to require grad (a bool tensor cannot): the call must refuse it before reading it."""

  @staticmethod
  def __new__(cls, t):
    return torch.Tensor._make_subclass(cls, t)

  @property
  def requires_grad(self):
    return True


UNSERVED = [dict(causal=True), dict(window_size=(64, 0)), dict(softcap=30.0), dict(rotary_cos=torch.zeros(256, 32)), dict(rotary_sin=torch.zeros(256, 32)),
            dict(alibi_slopes=torch.zeros(16)), dict(cache_batch_idx=torch.zeros(2, dtype=torch.int32)), dict(cache_leftpad=torch.zeros(2, dtype=torch.int32)),
            dict(shared_prefix_len=64), dict(cascade=True)]


@pytest.mark.parametrize("kw", UNSERVED + [dict(cu_seqlens_q=torch.zeros(3, dtype=torch.int32))])
def test_unserved_keywords_of_the_uniform_call_raise_by_name(kw):
  with pytest.raises(NotImplementedError, match=f"ffpa_attn_with_kvcache_mla_tree does not support: {next(iter(kw))}"):
    _call(*_uni(), **kw)


def test_the_docstrings_name_what_is_not_served():
  for fn, extra in ((ffpa_attn_amd.ffpa_attn_with_kvcache_mla_tree, ("cu_seqlens_q", "ffpa_attn_varlen_with_kvcache_mla_tree")),
                    (ffpa_attn_amd.ffpa_attn_varlen_with_kvcache_mla_tree, ("positions", "max_seqlen_q"))):
    doc = fn.__doc__
    for word in ("NOT served", "causal", "window_size", "softcap", "cascade", "rotary_cos", "ALiBi", "cache_batch_idx", "cache_leftpad", "FP8", "more than 64",
                 "masks over the prefix", "O = 0, LSE = -inf", "pack_tree_mask", "Inference only") + extra:
      assert word in doc, (fn.__name__, word)


# ----------------------------------------------------------------------------- the ragged call
def _rag(lens=(1, 0, 3), hq=16, hkv=1, d=576, page=64, pages=4, device="cpu", dtype=torch.bfloat16):
  B, T = len(lens), sum(lens)
  q = torch.zeros(T, hq, d, dtype=dtype, device=device)
  pool = torch.zeros(B * pages, page, hkv, d, dtype=dtype, device=device)
  table = torch.arange(B * pages, dtype=torch.int32, device=device).view(B, pages)
  cu = torch.tensor([0] + [sum(lens[:i + 1]) for i in range(B)], dtype=torch.int32, device=device)
  cache = torch.zeros(B, dtype=torch.int32, device=device)
  mask = torch.ones(max(lens), max(lens), dtype=torch.bool, device=device).tril()
  return q, pool, table, cu, cache, mask


def _rcall(q, pool, table, cu, cache, mask, dv=512, max_q=3, **kw):
  kw.setdefault("softmax_scale", SCALE)
  return ffpa_attn_amd.ffpa_attn_varlen_with_kvcache_mla_tree(q, pool, dv, cu, max_q, cache, table, tree_mask=mask, **kw)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("paged", [True, False])
def test_the_ragged_call_runs_on_meta_tensors(dtype, paged):
  lens = [1, 0, 3, 5, 1, 40]
  q, pool, table, cu, cache, mask = _rag(lens, hq=128, device="meta", dtype=dtype)
  if not paged:
    pool, table = torch.empty(len(lens), 128, 1, 576, dtype=dtype, device="meta"), None
  kv = torch.empty(sum(lens), 1, 576, dtype=dtype, device="meta")
  for m in (mask, torch.empty(6, 64, 64, dtype=torch.bool, device="meta"), torch.empty(6, 40, dtype=torch.int64, device="meta")):
    for new in (None, kv):
      out = _rcall(q, pool, table, cu, cache, m, max_q=40, kv=new)
      assert out.shape == (50, 128, 512) and out.dtype == dtype and out.device.type == "meta"
      out, lse = _rcall(q, pool, table, cu, cache, m, max_q=40, kv=new, return_softmax_lse=True)
      assert out.shape == (50, 128, 512) and lse.shape == (128, 50) and lse.dtype == torch.float32
  out, lse = _rcall(q[:0], pool, table, cu, cache, mask, max_q=0, return_softmax_lse=True)
  assert out.shape == (0, 128, 512) and lse.shape == (128, 0)


def test_ragged_argument_errors_name_the_argument():
  q, pool, table, cu, cache, mask = _rag()
  for kw in ({}, {"softmax_scale": None}):
    with pytest.raises(TypeError, match=r"ffpa_attn_varlen_with_kvcache_mla_tree: softmax_scale is required"):
      ffpa_attn_amd.ffpa_attn_varlen_with_kvcache_mla_tree(q, pool, 512, cu, 3, cache, table, tree_mask=mask, **kw)
  with pytest.raises(NotImplementedError, match=r"\(576, 448\) is not built"):
    _rcall(q, pool, table, cu, cache, mask, dv=448)
  with pytest.raises(ValueError, match="q must be packed"):
    _rcall(q[None], pool, table, cu, cache, mask)
  with pytest.raises(ValueError, match="max_seqlen_q must be a host int"):
    _rcall(q, pool, table, cu, cache, mask, max_q=0)
  with pytest.raises(TypeError, match="cache_seqlens must be a tensor"):
    _rcall(q, pool, table, cu, 7, mask)
  for bad in (torch.ones(2, 2, dtype=torch.bool), torch.ones(65, 65, dtype=torch.bool), torch.ones(3, 2, dtype=torch.int64), torch.ones(1, 65, dtype=torch.int64)):
    with pytest.raises(ValueError, match=r"ffpa_attn_varlen_with_kvcache_mla_tree: tree_mask must be bool \[W, W\].*3 <= W <= 64"):
      _rcall(q, pool, table, cu, cache, bad)
  for bad in (torch.ones(2, 3, 3, dtype=torch.bool), torch.ones(2, 5, dtype=torch.int64)):
    with pytest.raises(ValueError, match=r"ffpa_attn_varlen_with_kvcache_mla_tree: .*B=3"):
      _rcall(q, pool, table, cu, cache, bad)
  kv = torch.zeros(4, 1, 576, dtype=torch.bfloat16)
  for i in range(3):
    args = [q, pool, kv]
    args[i] = args[i].clone().requires_grad_(True)
    with pytest.raises(NotImplementedError, match=f"ffpa_attn_varlen_with_kvcache_mla_tree is inference only: {('q', 'kv_cache', 'kv')[i]} requires grad"):
      _rcall(args[0], args[1], table, cu, cache, mask, kv=args[2])
  with pytest.raises(NotImplementedError, match="inference only: tree_mask requires grad"):
    _rcall(q, pool, table, cu, cache, _Grad(mask))


@pytest.mark.parametrize("kw", UNSERVED + [dict(positions=torch.zeros(4, dtype=torch.int32))])
def test_unserved_keywords_of_the_ragged_call_raise_by_name(kw):
  with pytest.raises(NotImplementedError, match=f"ffpa_attn_varlen_with_kvcache_mla_tree does not support: {next(iter(kw))}"):
    _rcall(*_rag(), **kw)


def test_the_two_plain_latent_calls_still_refuse_a_tree_mask():
  q, pool, table, mask = _uni()
  with pytest.raises(NotImplementedError, match="ffpa_attn_with_kvcache_mla does not support: tree_mask"):
    ffpa_attn_amd.ffpa_attn_with_kvcache_mla(q, pool, 512, cache_seqlens=7, block_table=table, softmax_scale=SCALE, tree_mask=mask)
  q, pool, table, cu, cache, mask = _rag()
  with pytest.raises(NotImplementedError, match="ffpa_attn_varlen_with_kvcache_mla does not support: tree_mask"):
    ffpa_attn_amd.ffpa_attn_varlen_with_kvcache_mla(q, pool, 512, cu, 3, cache, table, softmax_scale=SCALE, tree_mask=mask)


# ----------------------------------------------------------------------------- the op
def test_the_op_has_a_fake_and_marks_only_the_append_s_targets_written():
  i32 = lambda *s: torch.empty(s, dtype=torch.int32, device="meta")
  pool = torch.empty(40, 64, 1, 576, dtype=torch.float16, device="meta")
  q = torch.empty(12, 128, 576, dtype=torch.float16, device="meta")
  words = torch.empty(6, 4, dtype=torch.int64, device="meta")
  o, lse = torch.ops.ffpa_attn._mla_tree_fwd_hip(q, pool, 512, i32(7), i32(6), i32(6, 5), words, None, None, 4, 320, 0.07)
  assert o.shape == (12, 128, 512) and o.dtype == torch.float16 and lse.shape == (128, 12) and lse.dtype == torch.float32
  schema = torch.ops.ffpa_attn._mla_tree_fwd_hip.default._schema
  assert [a.name for a in schema.arguments] == ["q", "kv_cache", "head_dim_v", "cu_seqlens_q", "seqused_k", "block_table", "tree_words", "kv_new", "cache_seqlens",
                                                "max_seqlen_q", "max_seqlen_k", "softmax_scale", "num_splits"]
  written = [a.name for a in schema.arguments if a.alias_info is not None and a.alias_info.is_write]
  assert written == ["kv_cache", "seqused_k"], str(schema)  # (what the append in front writes: the same two as ffpa_attn::_mla_fwd_hip)
  plain = torch.ops.ffpa_attn._mla_fwd_hip.default._schema
  assert written == [a.name for a in plain.arguments if a.alias_info is not None and a.alias_info.is_write]
  with pytest.raises(NotImplementedError, match="has no implementation for device 'cpu'"):
    hip.mla_tree_forward(torch.zeros(1, 16, 576, dtype=torch.bfloat16), torch.zeros(1, 64, 1, 576, dtype=torch.bfloat16), 512, torch.zeros(2, dtype=torch.int32),
                         torch.zeros(1, dtype=torch.int32), torch.zeros(1, 1, dtype=torch.int32), 1, 64, SCALE, torch.ones(1, 1, dtype=torch.int64))
  with pytest.raises(ValueError, match="tree_words is required"):
    hip.mla_tree_forward(None, None, 512, None, None, None, 1, 64, SCALE, None)


# ----------------------------------------------------------------------------- the C ABI
_KEEP = []


def _buf():
  buf = (ctypes.c_char * 4096)()
  _KEEP.append(buf)
  return (ctypes.addressof(buf) + 15) & ~15


def _c_args(group, lens, hkv=1, max_k=512, causal=False, num_splits=1, flags=0, tokens=None, tree_over=None):
  """A well-formed tree latent call on host buffers (only the plan and the checks run on it) -> (the latent call's three arguments, the tree mask, owners)."""
  B, hq, d, dv = len(lens), group * hkv, 576, 512
  p = hip._varlen_params(torch.bfloat16, B, hq, hkv, d, max(lens), max_k, sum(lens), [(hq * d, d), (hkv * d, d), (hkv * d, d), (hq * dv, dv)], causal, SCALE, -1.0,
                         flags, num_splits)
  base = _buf()
  p.q = p.k = p.o = p.cu_seqlens_q = p.seqused_kv = base
  p.workspace, p.workspace_bytes = base, 0xFFFFFFFFFFFFFFFF
  pages = -(-max_k // 64)
  kv = hip._paged_kv(base, pages, pages, 64, B * pages, 64 * hkv * d, 0)
  m = hip._stamped(hip.FfpaMla)
  m.head_dim_v = dv
  tm = hip._stamped(hip.FfpaTreeMask)
  tm.bits, tm.tokens, tm.batch_stride = base, max(lens) if tokens is None else tokens, 0
  for k_, v_ in (tree_over or {}).items():
    setattr(tm, k_, v_)
  return (ctypes.byref(p), ctypes.byref(kv), ctypes.byref(m)), ctypes.byref(tm), (p, kv, m, tm)


def _tree_plan(lib, args, tm):
  plan, name, slots = (ctypes.c_int * 5)(), ctypes.create_string_buffer(200), ctypes.c_int(-1)
  assert lib.ffpa_attn_varlen_mla_tree_fwd_plan(*args, tm, plan) == 0, lib.ffpa_attn_last_error()
  assert lib.ffpa_attn_varlen_mla_tree_fwd_kernel(*args, tm, name, 200) == 0
  assert lib.ffpa_attn_varlen_mla_tree_fwd_compact_slots(*args, tm, ctypes.byref(slots)) == 0
  return list(plan), name.value.decode(), slots.value


def _mla_plan(lib, args):
  plan, name, slots = (ctypes.c_int * 5)(), ctypes.create_string_buffer(200), ctypes.c_int(-1)
  assert lib.ffpa_attn_varlen_mla_fwd_plan(*args, plan) == 0, lib.ffpa_attn_last_error()
  assert lib.ffpa_attn_varlen_mla_fwd_kernel(*args, name, 200) == 0
  assert lib.ffpa_attn_varlen_mla_fwd_compact_slots(*args, ctypes.byref(slots)) == 0
  return list(plan), name.value.decode(), slots.value


PLAN_TABLE = [
  (1, [5] * 4), (1, [64] * 3),                                  # Hq == Hkv: unpacked
  (16, [1] * 8), (16, [3] * 8), (16, [4] * 8),                   # packed, one tile
  (16, [5] * 8), (128, [1] * 8), (128, [3] * 8), (16, [64] * 2),  # packed, chunked (a boundary inside a head at 16 x 5 and 128 x 3)
  (16, [1, 3, 0, 64, 7]), (16, [1] * 40 + [33]), (128, [1, 0, 3, 5, 1, 40]), (128, [1] * 20 + [16]),  # ragged: the full and the compact grid
]


@pytest.mark.parametrize("group, lens", PLAN_TABLE)
@pytest.mark.parametrize("hkv", [1, 2])
@pytest.mark.parametrize("splits, flags", [(1, 0), (0, 0), (3, "force"), (5, "force")])
def test_the_c_plan_is_the_latent_call_s_under_the_causal_flag(lib, group, lens, hkv, splits, flags, monkeypatch):
  monkeypatch.setenv("FFPA_HIP_FAKE_CUS", "256")
  fl = hip.FLAG_FORCE_SPLITS if flags == "force" else 0
  for max_k in (512, 16384):
    for caller_causal in (False, True):  # (the tree call ignores the caller's flag)
      args, tm, keep = _c_args(group, lens, hkv, max_k=max_k, causal=caller_causal, num_splits=splits, flags=fl)
      plan, name, slots = _tree_plan(lib, args, tm)
      cargs, _, ckeep = _c_args(group, lens, hkv, max_k=max_k, causal=True, num_splits=splits, flags=fl)
      want, want_name, want_slots = _mla_plan(lib, cargs)
      assert plan == want and slots == want_slots, (plan, want, slots, want_slots)
      assert name.startswith("ffpa_fwd_m16_mla_tree_kernel<bf16, 576, dv=512"), name
      assert name == want_name.replace("ffpa_fwd_m16_mla_kernel", "ffpa_fwd_m16_mla_tree_kernel")
      assert slots == hip.mla_compact_slots(group, lens)
      if flags == "force":
        assert plan[4] == splits and "ffpa_varlen_merge_kernel" in name
      ws = lib.ffpa_attn_varlen_mla_tree_fwd_workspace_bytes(*args, tm)
      assert ws == lib.ffpa_attn_varlen_mla_fwd_workspace_bytes(*cargs)
  assert (16, [1] * 40 + [33]) in PLAN_TABLE and hip.mla_compact_slots(16, [1] * 40 + [33]) > 0  # (the GPU suite's compact-grid batch)


def test_the_kernel_query_names_the_new_kernel_in_both_dtypes(lib):
  args, tm, keep = _c_args(128, [3] * 4)
  name = ctypes.create_string_buffer(200)
  assert lib.ffpa_attn_varlen_mla_tree_fwd_kernel(*args, tm, name, 200) == 0
  assert name.value.decode() == "ffpa_fwd_m16_mla_tree_kernel<bf16, 576, dv=512> (heads packed into rows, chunked)"
  keep[0].dtype = 1
  assert lib.ffpa_attn_varlen_mla_tree_fwd_kernel(*args, tm, name, 200) == 0
  assert name.value.decode().startswith("ffpa_fwd_m16_mla_tree_kernel<fp16, 576, dv=512>")
  keep[0].flags |= hip.FLAG_KV_STREAM
  assert lib.ffpa_attn_varlen_mla_tree_fwd_kernel(*args, tm, name, 200) == 0
  assert name.value.decode().startswith("ffpa_fwd_m16_mla_tree_kernel<fp16, 576, dv=512, NT>")
  assert lib.ffpa_attn_varlen_mla_tree_fwd_kernel(*args, tm, None, 0) == 1 and b"buf is NULL" in lib.ffpa_attn_last_error()


@pytest.mark.parametrize("over, status, text", [
  (dict(struct_size=24), 10, b"ffpa_tree_mask ABI mismatch"),
  (dict(struct_size=0), 10, b"ffpa_tree_mask ABI mismatch"),
  (dict(bits=None), 1, b"tree mask bits must be non-NULL"),
  (dict(tokens=0), 4, b"tokens=0 is outside [1, 64]"),
  (dict(tokens=65), 4, b"tokens=65 is outside [1, 64]"),
  (dict(tokens=4), 4, b"max_seqlen_q=5 exceeds the tree mask's tokens=4"),
  (dict(batch_stride=3), 5, b"batch_stride=3 is neither 0"),
])
def test_a_bad_tree_mask_is_refused_with_an_error_text_before_any_device_work(lib, over, status, text):
  args, tm, keep = _c_args(16, [5] * 4, tree_over=over)
  plan = (ctypes.c_int * 5)()
  for call in (lambda: lib.ffpa_attn_varlen_mla_tree_fwd(*args, tm, None), lambda: lib.ffpa_attn_varlen_mla_tree_fwd_plan(*args, tm, plan)):
    assert call() == status
    assert text in lib.ffpa_attn_last_error(), lib.ffpa_attn_last_error()
  assert lib.ffpa_attn_varlen_mla_tree_fwd_workspace_bytes(*args, tm) == 0


def test_null_structs_and_the_latent_call_s_own_refusals(lib):
  args, tm, keep = _c_args(16, [5] * 4)
  assert lib.ffpa_attn_varlen_mla_tree_fwd(*args, None, None) == 1 and b"tree mask is NULL" in lib.ffpa_attn_last_error()
  assert lib.ffpa_attn_varlen_mla_tree_fwd(args[0], args[1], None, tm, None) == 1 and b"mla is NULL" in lib.ffpa_attn_last_error()
  assert lib.ffpa_attn_varlen_mla_tree_fwd(args[0], None, args[2], tm, None) == 1 and b"paged kv is NULL" in lib.ffpa_attn_last_error()
  assert lib.ffpa_attn_varlen_mla_tree_fwd(None, args[1], args[2], tm, None) == 1 and b"params is NULL" in lib.ffpa_attn_last_error()
  keep[3].bits += 4
  assert lib.ffpa_attn_varlen_mla_tree_fwd(*args, tm, None) == 6 and b"8-byte aligned" in lib.ffpa_attn_last_error()
  keep[3].bits -= 4
  keep[2].head_dim_v = 448
  assert lib.ffpa_attn_varlen_mla_tree_fwd(*args, tm, None) == 3 and b"(576, 448) is not built" in lib.ffpa_attn_last_error()
  keep[2].head_dim_v = 512
  keep[0].struct_size -= 8
  assert lib.ffpa_attn_varlen_mla_tree_fwd(*args, tm, None) == 10 and b"ffpa_varlen_fwd_params ABI mismatch" in lib.ffpa_attn_last_error()


def test_abi_version_stays_7_and_the_exports_are_declared(lib):
  assert hip.ABI_VERSION == 7 and lib.ffpa_attn_query(0) == 7
  header = open(os.path.join(ROOT, "include", "ffpa_attn.h")).read()
  for suffix in ("", "_workspace_bytes", "_plan", "_kernel", "_compact_slots"):
    name = "ffpa_attn_varlen_mla_tree_fwd" + suffix
    assert name in hip.EXPORTS and getattr(lib, name) is not None, name
    assert re.search(rf"^\s*(?:int|size_t)\s+{name}\s*\(", header, flags=re.M), name
  assert ctypes.sizeof(hip.FfpaTreeMask) == 32 and ctypes.sizeof(hip.FfpaMla) == 56  # (no new struct, the two it takes keep their layout)


# ----------------------------------------------------------------------------- the code objects
def _kernel_metadata():
  """``[(kernel, its metadata block)]`` of the four builds (bf16 / fp16 x plain / NT) from the device assembly build() keeps."""
  paths = glob.glob(os.path.join(ROOT, "ffpa_attn_amd", "csrc", "build", "temps_d576", "ffpa_mla_tree_inst*gfx950.s*"))
  assert paths, "no device assembly of ffpa_mla_tree_inst.hip in csrc/build/temps_d576 (python -m ffpa_attn_amd.build keeps it)"
  path = paths[0]
  text = (gzip.open(path, "rt") if path.endswith(".gz") else open(path)).read()
  meta = re.findall(r"\.name:\s+(_Z\w*ffpa_fwd_m16_mla_tree_kernel\w*)\n(.*?)\.wavefront_size", text, flags=re.S)
  assert len(meta) == 4, [m[0] for m in meta]
  return meta


def test_the_new_kernels_use_no_scratch_and_spill_nothing(lib):
  """The code object's metadata of all four builds: no private segment, no vector spills, no scalar spills (the latent kernel parks ten scalar values in VGPR lanes
  across its KV loop; this unit reads what the epilogue needs of the kernel's arguments again behind the loop instead), and no more registers than the latent
  kernel: its 312 unified vector registers, at most its 106 SGPRs."""
  for name, block in _kernel_metadata():
    assert re.search(r"\.private_segment_fixed_size:\s+0\b", block), name
    assert re.search(r"\.vgpr_spill_count:\s+0\b", block), name
    assert re.search(r"\.sgpr_spill_count:\s+0\b", block), (name, re.search(r"\.sgpr_spill_count:\s+\d+", block).group(0))
    assert int(re.search(r"\.vgpr_count:\s+(\d+)", block).group(1)) == 312 and int(re.search(r"\.sgpr_count:\s+(\d+)", block).group(1)) <= 106, name
