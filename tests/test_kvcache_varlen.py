"""``ffpa_attn_varlen_with_kvcache`` without a GPU: everything the public call refuses (on meta tensors: before any device is touched), the float64 reference of
the ragged step (tests/kvcache_varlen_ref.py) against per-sequence calls of the uniform references, the fake op's shapes, the C struct against its ctypes mirror,
every argument check of ffpa_attn_kvcache_append_varlen (they come before any device work), and the new kernel's ISA."""

import ctypes
import glob
import gzip
import os
import re
import subprocess

import pytest
import torch

import kvcache_ref as R
import kvcache_softcap_ref as S
import kvcache_varlen_ref as V
from ffpa_attn_amd import ffpa_attn_varlen_with_kvcache, hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
  if not hip.library_available():
    from ffpa_attn_amd import build

    build.build()
  return hip.load_library()


# ----------------------------------------------------------------------------- the public call's refusals
def _meta(*shape, dtype=torch.bfloat16):
  return torch.empty(*shape, dtype=dtype, device="meta")


_I32 = torch.int32


def _call(**kw):
  """A well-formed paged step on meta tensors (T 10 over B 3, Hq 8 / Hkv 2, D 128, 4 pages of 64 per sequence, append + rotary + positions); each test breaks one
  argument."""
  pool = _meta(16, 64, 2, 128)
  args = dict(q=_meta(10, 8, 128), k_cache=pool, v_cache=pool, cu_seqlens_q=_meta(4, dtype=_I32), max_seqlen_q=5, cache_seqlens=_meta(3, dtype=_I32),
              block_table=_meta(3, 4, dtype=_I32), k=_meta(10, 2, 128), v=_meta(10, 2, 128), rotary_cos=_meta(256, 32), rotary_sin=_meta(256, 32),
              positions=_meta(10, dtype=_I32))
  args.update(kw)
  return ffpa_attn_varlen_with_kvcache(**args)


def test_the_well_formed_call_runs_on_meta_tensors():
  out, lse = _call(causal=True, return_softmax_lse=True)
  assert out.shape == (10, 8, 128) and out.dtype == torch.bfloat16 and lse.shape == (8, 10) and lse.dtype == torch.float32
  assert _call(window_size=(5, 0)).shape == (10, 8, 128) and _call(softcap=30.0, window_size=(5, 0)).shape == (10, 8, 128)
  # no token: empty tensors, nothing launched (a contiguous cache, whose attention launch is no registered op, would fail on meta otherwise)
  out, lse = _call(q=_meta(0, 8, 128), k=None, v=None, rotary_cos=None, rotary_sin=None, positions=None, max_seqlen_q=0, k_cache=_meta(3, 100, 2, 128),
                   v_cache=_meta(3, 100, 2, 128), block_table=None, return_softmax_lse=True)
  assert out.shape == (0, 8, 128) and lse.shape == (8, 0)


@pytest.mark.parametrize("kw, exc, text", [
  (dict(q=_meta(2, 5, 8, 128)), ValueError, r"q must be packed \[T, Hq, D\]"),
  (dict(q=_meta(10, 8, 128, dtype=torch.float32)), TypeError, "fp16/bf16 q/k_cache/v_cache"),
  (dict(q=_meta(10, 8, 64)), ValueError, "head dim of the cache"),
  (dict(q=_meta(10, 7, 128)), ValueError, "num_heads"),
  (dict(v_cache=_meta(16, 64, 4, 128)), ValueError, "k_cache .* and v_cache .* must share"),
  (dict(cu_seqlens_q=None), TypeError, "cu_seqlens_q must be a tensor"),
  (dict(cu_seqlens_q=_meta(4, dtype=torch.int64)), TypeError, "cu_seqlens_q must be int32"),
  (dict(cu_seqlens_q=_meta(1, dtype=_I32)), ValueError, "cu_seqlens_q must be a 1-D int32"),
  (dict(cu_seqlens_q=_meta(8, dtype=_I32)[::2]), ValueError, "cu_seqlens_q .* unit stride"),
  (dict(cu_seqlens_q=_meta(2, 2, dtype=_I32)), ValueError, "cu_seqlens_q"),
  (dict(max_seqlen_q=0), ValueError, "max_seqlen_q"),
  (dict(max_seqlen_q=2.0), ValueError, "max_seqlen_q"),
  (dict(max_seqlen_q=True), ValueError, "max_seqlen_q"),
  (dict(cache_seqlens=None), TypeError, "cache_seqlens must be a tensor"),
  (dict(cache_seqlens=7), TypeError, "cache_seqlens must be a tensor"),
  (dict(cache_seqlens=_meta(3, dtype=torch.int64)), TypeError, "cache_seqlens must be int32"),
  (dict(cache_seqlens=_meta(4, dtype=_I32)), ValueError, r"cache_seqlens must be an int32 tensor \[batch=3\]"),
  (dict(block_table=_meta(2, 4, dtype=_I32)), ValueError, r"block_table must be an int32 tensor \[batch=3"),
  (dict(block_table=_meta(3, 4, dtype=torch.int64)), ValueError, "block_table"),
  (dict(k_cache=_meta(16, 32, 2, 128), v_cache=_meta(16, 32, 2, 128)), ValueError, "page_size"),
  (dict(block_table=None), ValueError, r"k_cache \[B, capacity, Hkv, D\] must have cu_seqlens_q's batch \(3\)"),
  (dict(k=_meta(9, 2, 128), v=_meta(9, 2, 128)), ValueError, r"k must be \[T=10, Hkv=2, D=128\]"),
  (dict(v=_meta(10, 4, 128)), ValueError, r"v must be \[T=10, Hkv=2, D=128\]"),
  (dict(k=_meta(3, 4, 2, 128)), ValueError, r"k must be \[T=10"),
  (dict(k=_meta(10, 2, 128, dtype=torch.float16)), TypeError, "k must have the cache's dtype"),
  (dict(k=_meta(10, 2, 256)[..., ::2]), ValueError, "k must have a contiguous last dimension"),
  (dict(rotary_cos=_meta(256, 12), rotary_sin=_meta(256, 12)), ValueError, "rotary_dim"),
  (dict(rotary_cos=_meta(256, 72), rotary_sin=_meta(256, 72)), ValueError, "rotary_dim"),
  (dict(rotary_cos=_meta(255, 32), rotary_sin=_meta(255, 32)), ValueError, "seqlen_ro"),
  (dict(rotary_cos=_meta(256, 32, dtype=torch.float32)), TypeError, "rotary_cos must have q's dtype"),
  (dict(rotary_sin=_meta(256, 16)), ValueError, "share their shape"),
  (dict(positions=_meta(10, dtype=torch.int64)), TypeError, "positions must be an int32 tensor"),
  (dict(positions=[0] * 10), TypeError, "positions must be an int32 tensor"),
  (dict(positions=_meta(9, dtype=_I32)), ValueError, r"positions must be int32 \[T=10\]"),
  (dict(positions=_meta(2, 5, dtype=_I32)), ValueError, r"positions must be int32 \[T=10\]"),
  (dict(positions=_meta(20, dtype=_I32)[::2]), ValueError, "positions .* unit stride"),
  (dict(num_splits=-1), ValueError, "num_splits"),
  # window_size and softcap: the errors of _window_pair and of the softcap call
  (dict(window_size=None), TypeError, "window_size must be a pair of ints"),
  (dict(window_size=(1, 2, 3)), TypeError, "window_size must be a pair of ints"),
  (dict(window_size=(1.0, 0)), TypeError, "window_size must be a pair of ints"),
  (dict(window_size=(-2, 0)), ValueError, "window_size"),
  (dict(softcap="30"), TypeError, "softcap must be a real number"),
  (dict(softcap=True), TypeError, "softcap must be a real number"),
  (dict(softcap=-1.0), ValueError, "softcap"),
  (dict(softcap=float("nan")), ValueError, "softcap"),
  (dict(softcap=float("inf")), ValueError, "softcap"),
])
def test_argument_errors_name_the_argument(kw, exc, text):
  with pytest.raises(exc, match=text):
    _call(**kw)


@pytest.mark.parametrize("kw, names", [
  (dict(v=None), ["k"]),
  (dict(k=None), ["v"]),
  (dict(k=None, v=None), ["rotary_cos", "rotary_sin", "positions"]),
  (dict(rotary_sin=None), ["rotary_cos", "positions"]),
  (dict(rotary_cos=None), ["rotary_sin", "positions"]),
  (dict(rotary_cos=None, rotary_sin=None), ["positions"]),
])
def test_what_needs_another_argument_is_refused_by_name(kw, names):
  with pytest.raises(NotImplementedError) as e:
    _call(**kw)
  assert "does not support" in str(e.value)
  for n in names:
    assert n in str(e.value)


@pytest.mark.parametrize("name", ["q", "k_cache", "v_cache", "k", "v"])
def test_inference_only(name):
  shape = dict(q=(10, 8, 128), k_cache=(16, 64, 2, 128), v_cache=(16, 64, 2, 128), k=(10, 2, 128), v=(10, 2, 128))[name]
  t = torch.empty(shape, dtype=torch.bfloat16, device="meta", requires_grad=True)
  with pytest.raises(NotImplementedError, match=f"inference only: {name} requires grad"):
    _call(**{name: t})


def test_the_packed_call_keeps_refusing_block_table():
  from ffpa_attn_amd import ffpa_attn_varlen_func

  with pytest.raises((NotImplementedError, TypeError, ValueError)):
    ffpa_attn_varlen_func(_meta(10, 8, 128), _meta(10, 2, 128), _meta(10, 2, 128), _meta(4, dtype=_I32), _meta(4, dtype=_I32), 5, 5,
                          block_table=_meta(3, 4, dtype=_I32))


# ----------------------------------------------------------------------------- the fake op
@pytest.mark.parametrize("paged", [False, True])
@pytest.mark.parametrize("rotary", [False, True])
def test_fake_op_shapes_and_dtypes(paged, rotary):
  q, k = _meta(11, 32, 512), _meta(11, 8, 512)
  kc = _meta(40, 128, 8, 512) if paged else _meta(4, 640, 8, 512)
  bt = _meta(4, 5, dtype=_I32) if paged else None
  cos = _meta(640, 64) if rotary else None
  pos = _meta(11, dtype=_I32) if rotary else None
  q_rot, seqused = torch.ops.ffpa_attn._kvcache_append_varlen_hip(q, kc, kc, k, k, _meta(5, dtype=_I32), _meta(4, dtype=_I32), bt, cos, cos, pos, False, True)
  assert q_rot.shape == ((11, 32, 512) if rotary else (0,)) and q_rot.dtype == torch.bfloat16
  assert seqused.shape == (4,) and seqused.dtype == torch.int32


def test_the_op_schema_marks_the_caches_as_written():
  schema = torch.ops.ffpa_attn._kvcache_append_varlen_hip.default._schema
  assert [a.name for a in schema.arguments] == ["q", "k_cache", "v_cache", "k", "v", "cu_seqlens_q", "cache_seqlens", "block_table", "rotary_cos", "rotary_sin",
                                                "positions", "rotary_interleaved", "causal"]
  assert [a.name for a in schema.arguments if a.alias_info is not None and a.alias_info.is_write] == ["k_cache", "v_cache"]


def test_the_op_refuses_cpu_tensors_instead_of_falling_back():
  t = V.make_case([1, 2], [3, 4], D=64, page=0, seed=1)
  with pytest.raises(NotImplementedError):
    torch.ops.ffpa_attn._kvcache_append_varlen_hip(t["q"], t["k_cache"], t["v_cache"], t["k"], t["v"], t["cu"], t["lens"], None, None, None, None, True, False)


# ----------------------------------------------------------------------------- the reference
SEQS, LENS = [5, 1, 0, 3, 4], [0, 70, 9, 61, 126]


@pytest.mark.parametrize("page", [64, 0])
@pytest.mark.parametrize("interleaved, causal", [(True, True), (False, False)])
def test_reference_agrees_with_per_sequence_calls_of_the_uniform_reference(page, interleaved, causal):
  """Ragged append + attend against, per sequence, kvcache_ref.append on a batch of one followed by kvcache_ref.attend (plain), kvcache_window_ref.attend and
  kvcache_softcap_ref.attend: the same caches to the bit, the same outputs."""
  import kvcache_window_ref as W

  t = V.make_case(SEQS, LENS, D=64, page=page, seed=3, rotary_dim=32, pad=2)
  for window, softcap in (((-1, -1), 0.0), ((3, 0), 0.0), ((-1, -1), 30.0)):
    ref, kc, vc, rotated, used = V.reference(t, interleaved=interleaved, causal=causal, window=window, softcap=softcap)
    assert used == [5, 71, 9, 64, 130] and ref[0].shape == (1, 13, 8, 64) and ref[1].shape == (1, 8, 13)
    kc2, vc2 = t["k_cache"].clone(), t["v_cache"].clone()
    for b, (s, e) in enumerate(V.bounds(t["cu"])):
      one_k, one_v, tb = (kc2[b:b + 1], vc2[b:b + 1], None) if not page else (kc2, vc2, t["table"][b:b + 1])
      q_rot, u, _ = R.append(one_k, one_v, t["k"][s:e][None], t["v"][s:e][None], [LENS[b]], tb, t["cos"], t["sin"], interleaved, causal, q=t["q"][s:e][None])
      qb = q_rot.to(torch.bfloat16)
      if softcap:
        want = S.attend(qb, one_k, one_v, u, tb, window, causal, softcap=softcap)
      elif window != (-1, -1):
        want = W.attend(qb, one_k, one_v, u, tb, window, causal)
      else:
        want = R.attend(qb, one_k, one_v, u, tb, causal)
      assert torch.equal(ref[0][0, s:e], want[0][0]) and torch.equal(ref[1][0, :, s:e], want[1][0])
    assert torch.equal(kc.view(torch.int16), kc2.view(torch.int16)) and torch.equal(vc.view(torch.int16), vc2.view(torch.int16))
    # the padding rows were written nowhere: every row of the cache past the post-append lengths still holds NaN
    assert int(torch.isfinite(kc.float()).all(dim=-1).all(dim=-1).sum()) == sum(used)


def test_reference_positions_equal_the_default_at_the_slots_and_differ_for_a_tree():
  t = V.make_case(SEQS, LENS, D=64, page=64, seed=4, rotary_dim=64)
  slots = [LENS[b] + i for b in range(len(SEQS)) for i in range(SEQS[b])]
  default = V.reference(t, causal=True)
  at_slots = V.reference(t, causal=True, positions=torch.tensor(slots, dtype=torch.int32))
  assert all(torch.equal(a, b) for a, b in zip(default[0], at_slots[0]))
  assert torch.equal(default[1].view(torch.int16), at_slots[1].view(torch.int16)) and sorted(default[3]) == sorted(at_slots[3])
  depths = V.tree_depths(SEQS)
  assert depths == [0, 1, 1, 2, 2, 0, 0, 1, 1, 0, 1, 1, 2]
  tree = V.reference(t, causal=True, positions=torch.tensor([LENS[b] + d for b, d in zip(sum(([b] * n for b, n in enumerate(SEQS)), []), depths)], dtype=torch.int32))
  assert sorted(tree[3]) == sorted(default[3])  # the same slots are written ...
  assert not torch.equal(tree[1].view(torch.int16), default[1].view(torch.int16))  # ... with other keys
  eff = default[4]
  with pytest.raises(AssertionError):
    R.check(tree[0][0].to(torch.bfloat16), None, default[0], v=R.visible_values(default[2], eff, t["table"]), dtype="bf16")
  # positions are clamped to [0, seqlen_ro - 1]
  ro = t["cos"].size(0)
  wild = V.reference(t, positions=torch.tensor([-5, 10 ** 6] * 6 + [-1], dtype=torch.int32))
  tame = V.reference(t, positions=torch.tensor([0, ro - 1] * 6 + [0], dtype=torch.int32))
  assert torch.equal(wild[1].view(torch.int16), tame[1].view(torch.int16)) and torch.equal(wild[0][0], tame[0][0])


# ----------------------------------------------------------------------------- the C call
def test_ctypes_mirror_of_the_varlen_append_params_matches_the_c_header(tmp_path):
  fields = [f[0] for f in hip.FfpaKvAppendVarlenParams._fields_]
  src = tmp_path / "layout.c"
  body = "".join(f'printf("{f} %zu\\n", offsetof(ffpa_kv_append_varlen_params, {f}));\n' for f in fields)
  src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ffpa_attn.h"\nint main(void){\n'
                 'printf("sizeof %zu\\n", sizeof(ffpa_kv_append_varlen_params));\nprintf("append %zu\\n", sizeof(ffpa_kv_append_params));\n'
                 'printf("abi %d\\n", FFPA_ATTN_ABI_VERSION);\n' + body + "return 0;}\n")
  exe = tmp_path / "layout"
  subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
  out = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
  assert int(out["sizeof"]) == ctypes.sizeof(hip.FfpaKvAppendVarlenParams) == 264
  for f in fields:
    assert int(out[f]) == getattr(hip.FfpaKvAppendVarlenParams, f).offset, f
  assert int(out["append"]) == ctypes.sizeof(hip.FfpaKvAppendParams) == 280 and int(out["abi"]) == 7  # (no existing struct changed)


def test_the_symbol_is_exported_and_declared(lib):
  assert hip.ABI_VERSION == 7 and lib.ffpa_attn_query(0) == 7
  assert "ffpa_attn_kvcache_append_varlen" in hip.EXPORTS and lib.ffpa_attn_kvcache_append_varlen is not None
  header = open(os.path.join(ROOT, "include", "ffpa_attn.h")).read()
  assert set(re.findall(r"^\s*(?:int|size_t|const char\*)\s+(ffpa_attn_\w+)\s*\(", header, flags=re.M)) == set(hip.EXPORTS)


def _params(**over):
  """A well-formed ragged step (B 3, T 6, Hq 8 / Hkv 2, D 512, NeoX rotary over 128 dims, positions, contiguous cache of 1024) on a host buffer: only the argument
  checks run on it — each test breaks one argument."""
  p = hip.FfpaKvAppendVarlenParams()
  p.struct_size = ctypes.sizeof(hip.FfpaKvAppendVarlenParams)
  p.abi_version = hip.ABI_VERSION
  buf = (ctypes.c_char * 4096)()
  base = (ctypes.addressof(buf) + 15) & ~15
  p.q = p.k = p.v = p.k_cache = p.v_cache = p.q_rot = p.rotary_cos = p.rotary_sin = base
  p.seqused, p.cache_seqlens, p.cu_seqlens_q, p.positions = base + 16, base + 32, base + 48, base + 64
  p.batch, p.heads_q, p.heads_kv, p.head_dim, p.total_q = 3, 8, 2, 512, 6
  p.capacity, p.seqlen_ro = 1024, 1024
  p.q_stride[:] = p.q_rot_stride[:] = [8 * 512, 512]
  p.k_stride[:] = p.v_stride[:] = [2 * 512, 512]
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
  (dict(struct_size=256), 10, b"ffpa_kv_append_varlen_params ABI mismatch"),
  (dict(abi_version=6), 10, b"ABI mismatch"),
  (dict(dtype=2), 2, b"dtype"),
  (dict(batch=0), 4, b"non-positive"),
  (dict(heads_kv=3), 4, b"num_heads"),
  (dict(head_dim=100), 3, b"headdim not support"),
  (dict(head_dim=1032), 3, b"headdim not support"),
  (dict(total_q=-1), 4, b"total_q"),
  (dict(capacity=0), 4, b"capacity"),
  (dict(rotary_dim=24), 4, b"rotary_dim"),
  (dict(rotary_dim=528), 4, b"rotary_dim"),
  (dict(rotary_dim=-16), 4, b"rotary_dim"),
  (dict(seqlen_ro=1023), 4, b"seqlen_ro"),
  (dict(k_cache=None), 1, b"k_cache"),
  (dict(v_cache=None), 1, b"v_cache"),
  (dict(seqused=None), 1, b"seqused"),
  (dict(cache_seqlens=None), 1, b"cache_seqlens"),
  (dict(cu_seqlens_q=None), 1, b"cu_seqlens_q"),
  (dict(k=None), 1, b"k / v"),
  (dict(v=None), 1, b"k / v"),
  (dict(q=None), 1, b"q / q_rot"),
  (dict(q_rot=None), 1, b"q_rot"),
  (dict(rotary_cos=None), 1, b"rotary_cos"),
  (dict(rotary_sin=None), 1, b"rotary_sin"),
  (dict(rotary_dim=0), 4, b"positions"),
  (dict(k_stride=[-1024, 512]), 5, b"negative"),
  (dict(v_cache_stride=[1024 * 2 * 512, 2 * 512 + 4, 512]), 5, b"multiple of 8"),
  (dict(q_rot_stride=[4096, 500]), 5, b"multiple of 8"),
])
def test_status_codes_of_the_varlen_append_come_before_any_device_work(lib, over, status, text):
  p = _params(**over)
  assert lib.ffpa_attn_kvcache_append_varlen(ctypes.byref(p), None, None) == status
  assert text in lib.ffpa_attn_last_error(), lib.ffpa_attn_last_error()


def test_misaligned_and_aliased_pointers_of_the_varlen_append(lib):
  for name, add in (("k_cache", 8), ("v", 8), ("q", 8), ("q_rot", 4), ("rotary_cos", 8), ("seqused", 2), ("cache_seqlens", 1), ("cu_seqlens_q", 2), ("positions", 1)):
    p = _params()
    setattr(p, name, getattr(p, name) + add)
    assert lib.ffpa_attn_kvcache_append_varlen(ctypes.byref(p), None, None) == 6, name
    assert b"aligned" in lib.ffpa_attn_last_error()
  p = _params()
  p.seqused = p.cache_seqlens
  assert lib.ffpa_attn_kvcache_append_varlen(ctypes.byref(p), None, None) == 4 and b"seqused must not" in lib.ffpa_attn_last_error()
  assert lib.ffpa_attn_kvcache_append_varlen(None, None, None) == 1
  # what the call does not need is not checked: no rotary — q / q_rot / the tables are not read; no token row — k / v are not read.  Each call is then refused by
  # a check placed after those (the seqused / cache_seqlens alias)
  for over in (dict(rotary_dim=0, positions=None, q=None, q_rot=None, rotary_cos=None, rotary_sin=None, seqlen_ro=0, q_stride=[3, 3]),
               dict(total_q=0, k=None, v=None, q=None, q_rot=None, k_stride=[1, 1])):
    p = _params(**over)
    p.seqused = p.cache_seqlens
    assert lib.ffpa_attn_kvcache_append_varlen(ctypes.byref(p), None, None) == 4 and b"seqused must not" in lib.ffpa_attn_last_error(), over


@pytest.mark.parametrize("kv_over, status, text", [
  (dict(struct_size=48), 10, b"ffpa_paged_kv ABI mismatch"),
  (dict(block_table=None), 1, b"block_table"),
  (dict(page_size=32), 4, b"page_size"),
  (dict(page_size=96), 4, b"page_size"),
  (dict(num_pages=0), 4, b"num_pages"),
  (dict(bt_stride=8), 5, b"bt_stride"),
])
def test_status_codes_of_the_paged_varlen_append(lib, kv_over, status, text):
  p = _params()
  assert lib.ffpa_attn_kvcache_append_varlen(ctypes.byref(p), ctypes.byref(_pool(p, **kv_over)), None) == status
  assert text in lib.ffpa_attn_last_error(), lib.ffpa_attn_last_error()
  # (capacity is ignored when paged: pages_per_row x page_size = 1024 keys, and seqlen_ro must cover them)
  p = _params(capacity=0, seqlen_ro=1000)
  assert lib.ffpa_attn_kvcache_append_varlen(ctypes.byref(p), ctypes.byref(_pool(p)), None) == 4 and b"capacity 1024" in lib.ffpa_attn_last_error()


def test_varlen_append_kernel_isa_moves_16_byte_rows_without_scratch():
  """The kernel's device assembly (build() keeps it, gzip-compressed, in csrc/build/temps_append_varlen): every instantiation (bf16 / fp16 x interleaved / NeoX)
  moves K / V / q rows with 16-byte loads and stores, uses no scratch and spills nothing.  The search of cu_seqlens_q is the kernel's first loop: it must read
  cu_q with a scalar load and hold no vector load and no readfirstlane; and the kernel's only one-dword vector load is cache_seqlens[s] of the used[] write —
  cu_q[b], cache_seqlens[b], the page id and positions[t] are scalar loads too (they sit in front of the kernel's first store: behind it the compiler reads
  them with a vector load and a readfirstlane each)."""
  paths = glob.glob(os.path.join(ROOT, "ffpa_attn_amd", "csrc", "build", "temps_append_varlen", "*gfx950.s*"))
  if not paths:
    pytest.skip("no device assembly in csrc/build/temps_append_varlen (python -m ffpa_attn_amd.build keeps it)")
  path = paths[0]
  text = (gzip.open(path, "rt") if path.endswith(".gz") else open(path)).read()
  kernels = re.findall(r"^(_Z\w*ffpa_kv_append_varlen_kernel\w*):", text, flags=re.M)
  assert len(kernels) == 4, kernels
  for k in kernels:
    body = text.split(f"\n{k}:", 1)[1].split(".Lfunc_end", 1)[0]
    assert "scratch_" not in body, k
    loads = re.findall(r"global_load_(dword\w*)", body)
    stores = re.findall(r"global_store_(dword\w*)", body)
    assert loads.count("dwordx4") >= 2 and stores.count("dwordx4") >= 2, (k, loads, stores)
    assert all(w in ("dword", "dwordx2", "dwordx4") for w in loads + stores), (k, loads, stores)
    assert stores.count("dword") <= 1, (k, stores)  # (used[])
    assert loads.count("dword") <= 1, (k, loads)  # (cache_seqlens[s] of the used[] write: every wave-uniform read is a scalar load)
    # the first loop of the kernel (a label with a conditional branch back to it) is the binary search
    loops = [m for m in re.finditer(r"^(\.LBB\d+_\d+):.*?^\s+s_cbranch_\w+\s+\1\s*$", body, flags=re.M | re.S)]
    assert loops, k
    search = loops[0].group(0)
    first_store = body.index("global_store_dword")
    assert loops[0].end() < first_store, k
    assert re.search(r"^\s+s_load_dword\s", search, flags=re.M), (k, search)
    assert "global_load" not in search and "v_readfirstlane" not in search and "flat_load" not in search, (k, search)
    # ... and behind it, still in front of the first store: cu_q[b], cache_seqlens[b], the page id, positions[t]
    assert len(re.findall(r"^\s+s_load_dword\s", body[loops[0].end():first_store], flags=re.M)) >= 4, k
  meta = re.findall(r"\.name:\s+(_Z\w*ffpa_kv_append_varlen_kernel\w*)(.*?)\.wavefront_size", text, flags=re.S)
  assert len(meta) == 4
  for name, block in meta:
    assert re.search(r"\.private_segment_fixed_size:\s+0\b", block), name
    assert re.search(r"\.vgpr_spill_count:\s+0\b", block) and re.search(r"\.sgpr_spill_count:\s+0\b", block), name
