"""The tree-mask entry points of the C ABI without a GPU: ``ffpa_tree_mask`` against its ctypes mirror and gcc, the ABI pins, every refusal of
ffpa_attn_varlen_tree_fwd (they come before any device work) with its status and text, and the plan / kernel-name queries.  (There is no dropout refusal to
test: ``ffpa_varlen_fwd_params`` has no dropout field, so the packed call and the tree call cannot be asked for dropout at all.)"""

import ctypes
import os
import re
import subprocess

import pytest

from ffpa_attn_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
  if not hip.library_available():
    from ffpa_attn_amd import build

    build.build()
  return hip.load_library()


def test_ctypes_mirror_of_the_tree_mask_matches_the_c_header(tmp_path):
  fields = [f[0] for f in hip.FfpaTreeMask._fields_]
  src = tmp_path / "layout.c"
  body = "".join(f'printf("{f} %zu\\n", offsetof(ffpa_tree_mask, {f}));\n' for f in fields)
  src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ffpa_attn.h"\nint main(void){\n'
                 'printf("sizeof %zu\\n", sizeof(ffpa_tree_mask));\n'
                 'printf("varlen %zu\\n", sizeof(ffpa_varlen_fwd_params));\nprintf("paged %zu\\n", sizeof(ffpa_paged_kv));\n'
                 'printf("append %zu\\n", sizeof(ffpa_kv_append_params));\nprintf("merge %zu\\n", sizeof(ffpa_merge_states_params));\n'
                 'printf("abi %d\\n", FFPA_ATTN_ABI_VERSION);\n' + body + "return 0;}\n")
  exe = tmp_path / "layout"
  subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
  out = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
  assert int(out["sizeof"]) == ctypes.sizeof(hip.FfpaTreeMask) == 32
  for f in fields:
    assert int(out[f]) == getattr(hip.FfpaTreeMask, f).offset, f
  # the existing layouts and the ABI version stay where they were
  assert int(out["varlen"]) == ctypes.sizeof(hip.FfpaVarlenFwdParams) == 216 and int(out["paged"]) == ctypes.sizeof(hip.FfpaPagedKv) == 56
  assert int(out["append"]) == ctypes.sizeof(hip.FfpaKvAppendParams) and int(out["merge"]) == ctypes.sizeof(hip.FfpaMergeStatesParams) == 144
  assert int(out["abi"]) == 7


TREE_SYMBOLS = ("ffpa_attn_varlen_tree_fwd", "ffpa_attn_varlen_tree_fwd_plan", "ffpa_attn_varlen_tree_fwd_kernel", "ffpa_attn_varlen_tree_fwd_workspace_bytes")


def test_abi_version_stays_7_and_the_symbols_are_exported(lib):
  assert hip.ABI_VERSION == 7 and lib.ffpa_attn_query(0) == 7
  for name in TREE_SYMBOLS:
    assert name in hip.EXPORTS and getattr(lib, name) is not None, name
  header = open(os.path.join(ROOT, "include", "ffpa_attn.h")).read()
  declared = set(re.findall(r"^\s*(?:int|size_t|const char\*)\s+(ffpa_attn_\w+)\s*\(", header, flags=re.M))
  assert declared == set(hip.EXPORTS)
  # the ops whose schemas the serving calls depend on are what they were
  import torch

  names = lambda op: [a.name for a in op.default._schema.arguments]
  assert names(torch.ops.ffpa_attn._paged_fwd_hip) == ["q", "k", "v", "cu_seqlens_q", "seqused_k", "block_table", "max_seqlen_q", "max_seqlen_k", "softmax_scale",
                                                      "causal", "rescale_threshold", "num_splits"]
  assert names(torch.ops.ffpa_attn._kvcache_append_hip) == ["q", "k_cache", "v_cache", "k", "v", "cache_seqlens", "block_table", "rotary_cos", "rotary_sin",
                                                           "rotary_interleaved", "causal"]
  assert names(torch.ops.ffpa_attn._merge_states_hip) == ["o_a", "lse_a", "o_b", "lse_b"]
  assert "tree_words" in names(torch.ops.ffpa_attn._tree_fwd_hip)


_KEEP = []


def _buf():
  buf = (ctypes.c_char * 4096)()
  _KEEP.append(buf)
  return (ctypes.addressof(buf) + 15) & ~15


def _call_args(d=512, paged=True, sq=4, over=None, tree_over=None, no_tree=False):
  """A well-formed tree call on host buffers (only the argument checks and the plan run on it) -> the ctypes arguments (p, kv | None, tree | None)."""
  hq, hkv, B = 8, 2, 3
  p = hip._varlen_params(__import__("torch").bfloat16, B, hq, hkv, d, sq, 4096, B * sq, [(hq * d, d), (hkv * d, d), (hkv * d, d), (hq * d, d)], False, d ** -0.5, -1.0, 0, 0)
  base = _buf()
  p.q = p.k = p.v = p.o = p.cu_seqlens_q = p.cu_seqlens_kv = p.seqused_kv = base
  for k_, v_ in (over or {}).items():
    setattr(p, k_, v_)
  kv = hip._paged_kv(base, 64, 64, 64, 192, 64 * hkv * d, 64 * hkv * d) if paged else None
  tree = hip._stamped(hip.FfpaTreeMask)
  tree.bits, tree.tokens, tree.batch_stride = base, sq, sq
  for k_, v_ in (tree_over or {}).items():
    setattr(tree, k_, v_)
  return ctypes.byref(p), (ctypes.byref(kv) if paged else None), (None if no_tree else ctypes.byref(tree)), (p, kv, tree)


@pytest.mark.parametrize("paged", [True, False])
@pytest.mark.parametrize("kw, status, text", [
  (dict(no_tree=True), 1, b"tree mask is NULL"),
  (dict(tree_over=dict(bits=None)), 1, b"tree mask bits must be non-NULL"),
  (dict(tree_over=dict(struct_size=24)), 10, b"ffpa_tree_mask ABI mismatch"),
  (dict(tree_over=dict(struct_size=0)), 10, b"ffpa_tree_mask ABI mismatch"),
  (dict(tree_over=dict(tokens=0)), 4, b"outside [1, 64]"),
  (dict(tree_over=dict(tokens=-3)), 4, b"outside [1, 64]"),
  (dict(tree_over=dict(tokens=65)), 4, b"outside [1, 64]"),
  (dict(tree_over=dict(tokens=3)), 4, b"max_seqlen_q=4 exceeds the tree mask's tokens=3"),
  (dict(sq=65, tree_over=dict(tokens=64)), 4, b"max_seqlen_q=65 exceeds the tree mask's tokens=64"),
  (dict(tree_over=dict(batch_stride=3)), 5, b"batch_stride"),
  (dict(tree_over=dict(batch_stride=-4)), 5, b"batch_stride"),
  # the packed call's own refusals come first
  (dict(over=dict(dtype=2)), 2, b"dtype"),
  (dict(over=dict(head_dim=1032)), 3, b"headdim not support"),
  (dict(over=dict(abi_version=6)), 10, b"ffpa_varlen_fwd_params ABI mismatch"),
  (dict(over=dict(heads_kv=3)), 4, b"num_heads"),
])
def test_status_codes_of_the_tree_call_come_before_any_device_work(lib, paged, kw, status, text):
  p, kv, tree, keep = _call_args(paged=paged, **kw)
  for fn, extra in ((lib.ffpa_attn_varlen_tree_fwd, (None,)), (lib.ffpa_attn_varlen_tree_fwd_plan, ((ctypes.c_int * 5)(),)),
                    (lib.ffpa_attn_varlen_tree_fwd_kernel, (ctypes.create_string_buffer(200), 200))):
    assert fn(p, kv, tree, *extra) == status, fn
    assert text in lib.ffpa_attn_last_error(), lib.ffpa_attn_last_error()


def test_misaligned_bits_and_a_bad_pool_of_the_tree_call(lib):
  p, kv, tree, keep = _call_args()
  keep[2].bits += 4
  assert lib.ffpa_attn_varlen_tree_fwd(p, kv, tree, None) == 6 and b"8-byte aligned" in lib.ffpa_attn_last_error()
  p, kv, tree, keep = _call_args()
  keep[1].page_size = 48
  assert lib.ffpa_attn_varlen_tree_fwd(p, kv, tree, None) == 4 and b"page_size" in lib.ffpa_attn_last_error()
  # a shared tree (batch_stride 0) and a padded one (batch_stride > tokens) pass the tree's checks: the plan answers
  for stride in (0, 64):
    p, kv, tree, keep = _call_args(tree_over=dict(batch_stride=stride))
    assert lib.ffpa_attn_varlen_tree_fwd_plan(p, kv, tree, (ctypes.c_int * 5)()) == 0, lib.ffpa_attn_last_error()
  assert lib.ffpa_attn_varlen_tree_fwd_workspace_bytes(p, kv, None) == 0


@pytest.mark.parametrize("paged", [True, False])
@pytest.mark.parametrize("d", [128, 512, 1024])
@pytest.mark.parametrize("sq", [1, 4, 64])
def test_plan_and_kernel_name_queries(lib, d, paged, sq):
  """The tree call's plan is the packed / paged call's own (one row tile per (sequence, head), the same tile, the same grid), its kernel the tree build of the same
  family — at one token per sequence too."""
  p, kv, tree, keep = _call_args(d=d, paged=paged, sq=sq)
  plan, name = (ctypes.c_int * 5)(), ctypes.create_string_buffer(200)
  assert lib.ffpa_attn_varlen_tree_fwd_plan(p, kv, tree, plan) == 0, lib.ffpa_attn_last_error()
  assert lib.ffpa_attn_varlen_tree_fwd_kernel(p, kv, tree, name, 200) == 0
  plain, plain_name = (ctypes.c_int * 5)(), ctypes.create_string_buffer(200)
  if paged:
    assert lib.ffpa_attn_varlen_paged_fwd_plan(p, kv, plain) == 0 and lib.ffpa_attn_varlen_paged_fwd_kernel(p, kv, plain_name, 200) == 0
  else:
    assert lib.ffpa_attn_varlen_fwd_plan(p, plain) == 0 and lib.ffpa_attn_varlen_fwd_kernel(p, plain_name, 200) == 0
  assert list(plan) == list(plain)
  assert plan[0] == 1 and plan[1] == (128 if d <= 512 else 64) and plan[2] == (64 if d <= 512 else 32)
  text = name.value.decode()
  assert text.startswith(f"ffpa_fwd_m16_{'paged' if paged else 'varlen'}_tree_kernel<bf16, {d}>")
  assert text.replace("_tree_kernel<", "_kernel<") == plain_name.value.decode()
  packed = 4 * sq <= plan[1]  # (group 4: the heads of a KV group x the tokens fit the tile's rows)
  assert ("(GQA heads packed into rows)" in text) == packed
