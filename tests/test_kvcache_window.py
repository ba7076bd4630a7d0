"""The sliding-window entry point without a GPU: the export and its argument errors, ``ffpa_window`` against its ctypes mirror and gcc, the ABI pins, every
refusal of ffpa_attn_varlen_window_fwd (they come before any device work), the plan — priced at the window's keys, not the capacity — and the float64
reference of the visibility rule (tests/kvcache_window_ref.py) against a brute-force loop."""

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
import kvcache_window_ref as W
from ffpa_attn_amd import ffpa_attn_with_kvcache, ffpa_attn_with_kvcache_window, hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
  if not hip.library_available():
    from ffpa_attn_amd import build

    build.build()
  return hip.load_library()


# ----------------------------------------------------------------------------- the Python entry
def test_the_entry_point_is_exported():
  assert "ffpa_attn_with_kvcache_window" in ffpa_attn_amd.__all__
  assert ffpa_attn_amd.ffpa_attn_with_kvcache_window is ffpa_attn_with_kvcache_window


def _cpu_args(B=2, sq=1, hq=8, hkv=2, d=128, cap=256):
  q = torch.zeros(B, sq, hq, d, dtype=torch.bfloat16)
  kc = torch.zeros(B, cap, hkv, d, dtype=torch.bfloat16)
  return q, kc, kc.clone()


def test_window_size_is_required_and_checked():
  q, kc, vc = _cpu_args()
  with pytest.raises(TypeError):
    ffpa_attn_with_kvcache_window(q, kc, vc, cache_seqlens=7)  # (keyword-only, no default)
  for bad in (None, 64, (64,), (1, 2, 3), "ab", (64, 2.0), (True, 0), (torch.tensor(3), 0)):
    with pytest.raises(TypeError, match="window_size must be a pair of ints"):
      ffpa_attn_with_kvcache_window(q, kc, vc, cache_seqlens=7, window_size=bad)
  for bad in ((-2, 0), (0, -2), (-5, -5)):
    with pytest.raises(ValueError, match="must be >= -1"):
      ffpa_attn_with_kvcache_window(q, kc, vc, cache_seqlens=7, window_size=bad)


def _raises_like_the_plain_call(kwargs_of, **kw):
  """What ``_kv_check`` refuses is refused by the window entry with the same exception type and text."""
  with pytest.raises(Exception) as plain:
    ffpa_attn_with_kvcache(*kwargs_of[0], **kwargs_of[1], **kw)
  with pytest.raises(type(plain.value)) as win:
    ffpa_attn_with_kvcache_window(*kwargs_of[0], **kwargs_of[1], **kw, window_size=(64, 0))
  assert str(win.value) == str(plain.value)


def test_what_validate_refuses_is_refused_with_the_same_text():
  q, kc, vc = _cpu_args()
  _raises_like_the_plain_call(((q.float(), kc, vc), {}))                                        # dtype
  _raises_like_the_plain_call(((q, kc, vc[:, :100]), {}))                                       # cache shapes
  _raises_like_the_plain_call(((q[0], kc, vc), {}))                                             # rank
  _raises_like_the_plain_call(((q[:, :, :3], kc, vc), {}))                                      # Hq % Hkv
  _raises_like_the_plain_call(((q, kc, vc), {}), num_splits=-1)
  _raises_like_the_plain_call(((q, kc, vc), {}), cache_seqlens=-4)
  _raises_like_the_plain_call(((q, kc, vc), {}), cache_seqlens=torch.zeros(5, dtype=torch.int32))
  _raises_like_the_plain_call(((q, kc, vc), {}), cache_seqlens="7")
  _raises_like_the_plain_call(((q, kc, vc), {}), block_table=torch.zeros(2, 4, dtype=torch.int64))
  _raises_like_the_plain_call(((q, kc, vc), {}), k=torch.zeros(2, 1, 2, 128, dtype=torch.bfloat16), cache_seqlens=3)               # k without v
  _raises_like_the_plain_call(((q, kc, vc), {}), rotary_cos=torch.zeros(256, 8, dtype=torch.bfloat16), cache_seqlens=3)          # rotary without k / v
  knew = torch.zeros(2, 1, 2, 128, dtype=torch.bfloat16)
  _raises_like_the_plain_call(((q, kc, vc), {}), k=knew, v=knew)                                # append without cache_seqlens
  _raises_like_the_plain_call(((q, kc, vc), {}), k=knew, v=knew[:, :, :1], cache_seqlens=3)     # new keys' shape


def test_a_tensor_that_requires_grad_raises():
  q, kc, vc = _cpu_args()
  for i in range(3):
    args = [q, kc, vc]
    args[i] = args[i].clone().requires_grad_(True)
    with pytest.raises(NotImplementedError, match="inference only"):
      ffpa_attn_with_kvcache_window(*args, cache_seqlens=7, window_size=(64, 0))


def test_the_existing_entries_keep_refusing_window_size():
  q, kc, vc = _cpu_args()
  with pytest.raises(NotImplementedError, match="window_size"):
    ffpa_attn_with_kvcache(q, kc, vc, cache_seqlens=7, window_size=(64, 0))


def test_the_op_has_a_fake_shaped_like_the_tree_ops():
  names = [a.name for a in torch.ops.ffpa_attn._window_fwd_hip.default._schema.arguments]
  assert names == ["q", "k", "v", "cu_seqlens_q", "cu_seqlens_k", "seqused_k", "block_table", "window_left", "window_right", "max_seqlen_q", "max_seqlen_k",
                   "softmax_scale", "causal", "rescale_threshold", "num_splits"]
  q = torch.empty(12, 8, 128, dtype=torch.bfloat16, device="meta")
  kv = torch.empty(40, 64, 2, 128, dtype=torch.bfloat16, device="meta")
  i32 = lambda *s: torch.empty(s, dtype=torch.int32, device="meta")
  o, lse = torch.ops.ffpa_attn._window_fwd_hip(q, kv, kv, i32(4), None, i32(3), i32(3, 8), 64, 0, 4, 512, 0.1, 1)
  assert o.shape == (12, 8, 128) and o.dtype == torch.bfloat16 and lse.shape == (8, 12) and lse.dtype == torch.float32


# ----------------------------------------------------------------------------- the C ABI
def test_ctypes_mirror_of_the_window_matches_the_c_header(tmp_path):
  fields = [f[0] for f in hip.FfpaWindow._fields_]
  src = tmp_path / "layout.c"
  body = "".join(f'printf("{f} %zu\\n", offsetof(ffpa_window, {f}));\n' for f in fields)
  src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ffpa_attn.h"\nint main(void){\n'
                 'printf("sizeof %zu\\n", sizeof(ffpa_window));\n'
                 'printf("varlen %zu\\n", sizeof(ffpa_varlen_fwd_params));\nprintf("paged %zu\\n", sizeof(ffpa_paged_kv));\n'
                 'printf("tree %zu\\n", sizeof(ffpa_tree_mask));\nprintf("abi %d\\n", FFPA_ATTN_ABI_VERSION);\n' + body + "return 0;}\n")
  exe = tmp_path / "layout"
  subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
  out = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
  assert int(out["sizeof"]) == ctypes.sizeof(hip.FfpaWindow) == 16
  assert fields == ["struct_size", "reserved", "left", "right"]
  for f in fields:
    assert int(out[f]) == getattr(hip.FfpaWindow, f).offset, f
  # the existing layouts and the ABI version stay where they were
  assert int(out["varlen"]) == ctypes.sizeof(hip.FfpaVarlenFwdParams) == 216 and int(out["paged"]) == ctypes.sizeof(hip.FfpaPagedKv) == 56
  assert int(out["tree"]) == ctypes.sizeof(hip.FfpaTreeMask) == 32 and int(out["abi"]) == 7


WINDOW_SYMBOLS = ("ffpa_attn_varlen_window_fwd", "ffpa_attn_varlen_window_fwd_plan", "ffpa_attn_varlen_window_fwd_kernel",
                  "ffpa_attn_varlen_window_fwd_workspace_bytes")


def test_abi_version_stays_7_and_the_four_symbols_are_exported(lib):
  assert hip.ABI_VERSION == 7 and lib.ffpa_attn_query(0) == 7
  for name in WINDOW_SYMBOLS:
    assert name in hip.EXPORTS and getattr(lib, name) is not None, name
  header = open(os.path.join(ROOT, "include", "ffpa_attn.h")).read()
  declared = set(re.findall(r"^\s*(?:int|size_t|const char\*)\s+(ffpa_attn_\w+)\s*\(", header, flags=re.M))
  assert declared == set(hip.EXPORTS)


_KEEP = []


def _buf():
  buf = (ctypes.c_char * 4096)()
  _KEEP.append(buf)
  return (ctypes.addressof(buf) + 15) & ~15


def _call_args(d=512, paged=True, sq=1, window=(4096, 0), B=32, hq=32, hkv=8, max_k=32768, causal=True, total_q=None, num_splits=0, over=None, win_over=None,
               no_window=False):
  """A well-formed window call on host buffers (only the argument checks and the plan run on it) -> the ctypes arguments (p, kv | None, w | None) + what owns them."""
  p = hip._varlen_params(torch.bfloat16, B, hq, hkv, d, sq, max_k, B * sq if total_q is None else total_q, [(hq * d, d), (hkv * d, d), (hkv * d, d), (hq * d, d)],
                         causal, d ** -0.5, -1.0, 0, num_splits)
  base = _buf()
  p.q = p.k = p.v = p.o = p.cu_seqlens_q = p.cu_seqlens_kv = p.seqused_kv = base
  p.workspace, p.workspace_bytes = base, 0xFFFFFFFFFFFFFFFF  # (a call that hands the library its scratch: the plan may split)
  for k_, v_ in (over or {}).items():
    setattr(p, k_, v_)
  pages = -(-max_k // 64)
  kv = hip._paged_kv(base, pages, pages, 64, B * pages, 64 * hkv * d, 64 * hkv * d) if paged else None
  w = hip._stamped(hip.FfpaWindow)
  w.left, w.right = window
  for k_, v_ in (win_over or {}).items():
    setattr(w, k_, v_)
  return ctypes.byref(p), (ctypes.byref(kv) if paged else None), (None if no_window else ctypes.byref(w)), (p, kv, w)


@pytest.mark.parametrize("paged", [True, False])
@pytest.mark.parametrize("kw, status, text", [
  (dict(no_window=True), 1, b"window is NULL"),
  (dict(win_over=dict(struct_size=12)), 10, b"ffpa_window ABI mismatch"),
  (dict(win_over=dict(struct_size=0)), 10, b"ffpa_window ABI mismatch"),
  (dict(win_over=dict(reserved=1)), 10, b"reserved"),
  (dict(window=(-2, 0)), 4, b"must be >= -1"),
  (dict(window=(0, -2)), 4, b"must be >= -1"),
  (dict(window=(-2147483648, -1)), 4, b"must be >= -1"),
  # the packed call's own refusals come first
  (dict(over=dict(dtype=2)), 2, b"dtype"),
  (dict(over=dict(head_dim=1032)), 3, b"headdim not support"),
  (dict(over=dict(abi_version=6)), 10, b"ffpa_varlen_fwd_params ABI mismatch"),
  (dict(over=dict(heads_kv=3)), 4, b"num_heads"),
])
def test_status_codes_of_the_window_call_come_before_any_device_work(lib, paged, kw, status, text):
  p, kv, w, keep = _call_args(paged=paged, **kw)
  for fn, extra in ((lib.ffpa_attn_varlen_window_fwd, (None,)), (lib.ffpa_attn_varlen_window_fwd_plan, ((ctypes.c_int * 5)(),)),
                    (lib.ffpa_attn_varlen_window_fwd_kernel, (ctypes.create_string_buffer(200), 200))):
    assert fn(p, kv, w, *extra) == status, fn
    assert text in lib.ffpa_attn_last_error(), lib.ffpa_attn_last_error()
  assert lib.ffpa_attn_varlen_window_fwd_workspace_bytes(p, kv, w) == 0


def _plans(lib, paged, **kw):
  """(window plan, window kernel name, owner)"""
  p, kv, w, keep = _call_args(paged=paged, **kw)
  plan, name = (ctypes.c_int * 5)(), ctypes.create_string_buffer(200)
  assert lib.ffpa_attn_varlen_window_fwd_plan(p, kv, w, plan) == 0, lib.ffpa_attn_last_error()
  assert lib.ffpa_attn_varlen_window_fwd_kernel(p, kv, w, name, 200) == 0
  return list(plan), name.value.decode(), (p, kv, keep)


def _plain(lib, paged, p, kv, max_k=None, causal=None):
  pp = p._obj if hasattr(p, "_obj") else p
  old = pp.max_seqlen_kv, pp.causal
  if max_k is not None:
    pp.max_seqlen_kv = max_k
  if causal is not None:
    pp.causal = causal
  plan, name = (ctypes.c_int * 5)(), ctypes.create_string_buffer(200)
  if paged:
    assert lib.ffpa_attn_varlen_paged_fwd_plan(p, kv, plan) == 0 and lib.ffpa_attn_varlen_paged_fwd_kernel(p, kv, name, 200) == 0
  else:
    assert lib.ffpa_attn_varlen_fwd_plan(p, plan) == 0 and lib.ffpa_attn_varlen_fwd_kernel(p, name, 200) == 0
  pp.max_seqlen_kv, pp.causal = old
  return list(plan), name.value.decode()


@pytest.mark.parametrize("paged", [True, False])
@pytest.mark.parametrize("d, hq, hkv", [(512, 32, 8), (1024, 16, 4)])
@pytest.mark.parametrize("B", [32, 4])
def test_the_plan_prices_the_window_not_the_capacity(lib, paged, d, hq, hkv, B, monkeypatch):
  """The varlen_decode family (B sequences x 1 token over a 32k cache): with left = 4096 the split count and the NT flag are the plain plan's at
  max_seqlen_k = 4096 + max_seqlen_q rounded up to a KV tile — and not the plain plan's at 32768.  The two plans must differ where the NT rule (K or V bytes
  with one reader >= 272 MiB) separates the lengths: B = 4 streams 4 x Hkv x L x D x 2 B = 1 GiB of K at 32768 keys and 130 MiB at 4160 (B = 32: 8 GiB and
  1 GiB, the same side of the rule, and the split count may agree too: only the equality is asserted there)."""
  monkeypatch.setenv("FFPA_HIP_FAKE_CUS", "256")  # (the plan of an MI355X, whatever runs the test)
  sq = 1
  plan, name, (p, kv, keep) = _plans(lib, paged, d=d, hq=hq, hkv=hkv, sq=sq, B=B, window=(4096, 0))
  bc = plan[2]
  priced = (4096 + sq + bc - 1) // bc * bc
  small, small_name = _plain(lib, paged, p, kv, max_k=priced)
  full, full_name = _plain(lib, paged, p, kv)
  nt = lambda text: ", NT>" in text
  assert plan == small and nt(name) == nt(small_name)
  assert name.replace("_window_kernel<", "_kernel<") == small_name
  if B == 4:
    assert nt(full_name) and not nt(name), (plan, name, full, full_name)
    assert (plan[4], nt(name)) != (full[4], nt(full_name))
  assert name.startswith(f"ffpa_fwd_m16_{'paged' if paged else 'varlen'}_window_kernel<bf16, {d}")
  # no left bound: the plan is the plain plan (non-causal (-1, -1); (-1, 0) and causal=True are the causal plan)
  keep[2].left, keep[2].right = -1, -1
  keep[0].causal = 0
  plan2, name2 = (ctypes.c_int * 5)(), ctypes.create_string_buffer(200)
  assert lib.ffpa_attn_varlen_window_fwd_plan(p, kv, ctypes.byref(keep[2]), plan2) == 0
  assert lib.ffpa_attn_varlen_window_fwd_kernel(p, kv, ctypes.byref(keep[2]), name2, 200) == 0
  plain, plain_name = _plain(lib, paged, p, kv, causal=0)
  assert list(plan2) == plain and name2.value.decode().replace("_window_kernel<", "_kernel<") == plain_name
  # a window at least as long as the cache is no window
  keep[2].left, keep[2].right = 32768, 0
  assert lib.ffpa_attn_varlen_window_fwd_plan(p, kv, ctypes.byref(keep[2]), plan2) == 0
  assert list(plan2) == _plain(lib, paged, p, kv, causal=1)[0]


def test_the_priced_length_of_a_prefill_chunk_and_the_workspace(lib, monkeypatch):
  """Several row tiles per head: a row tile of R rows sees at most left + min(max_seqlen_q, R + right) keys; the workspace query answers for that plan."""
  monkeypatch.setenv("FFPA_HIP_FAKE_CUS", "256")
  for right, causal in ((0, False), (16, False), (-1, False), (5, True)):
    plan, name, (p, kv, keep) = _plans(lib, True, d=512, B=1, hq=8, hkv=8, sq=1024, max_k=65536, window=(1000, right), causal=causal)
    br, bc = plan[1], plan[2]
    r_eff = 0 if causal else right
    tail = 1024 if r_eff < 0 else min(1024, br + r_eff)
    priced = (1000 + tail + bc - 1) // bc * bc
    assert plan == _plain(lib, True, p, kv, max_k=priced, causal=1 if r_eff >= 0 else 0)[0], (right, causal)
    ws = lib.ffpa_attn_varlen_window_fwd_workspace_bytes(p, kv, ctypes.byref(keep[2]))
    assert (ws > 0) == (plan[4] > 1)
    if plan[4] > 1:
      assert ws == plan[4] * 8 * 1024 * (512 + 1) * 4


# ----------------------------------------------------------------------------- the float64 reference
def _brute(q, k, v, n, window, causal, scale):
  """Softmax attention of one sequence by loops: q [sq, H, D], k / v [n, H, D] (MHA), python floats."""
  left, right = window
  if causal:
    right = 0
  sq, H, D = q.shape
  o = [[[0.0] * D for _ in range(H)] for _ in range(sq)]
  lse = [[-math.inf] * sq for _ in range(H)]
  for i in range(sq):
    pos = i + n - sq
    for h in range(H):
      scores = {}
      for j in range(n):
        if (left < 0 or j >= pos - left) and (right < 0 or j <= pos + right):
          scores[j] = sum(float(q[i, h, e]) * float(k[j, h, e]) for e in range(D)) * scale
      if not scores:
        continue
      m = max(scores.values())
      l = sum(math.exp(s - m) for s in scores.values())
      lse[h][i] = m + math.log(l)
      for e in range(D):
        o[i][h][e] = sum(math.exp(s - m) / l * float(v[j, h, e]) for j, s in scores.items())
  return torch.tensor(o, dtype=torch.float64), torch.tensor(lse, dtype=torch.float64)


@pytest.mark.parametrize("window, causal", [((-1, -1), False), ((-1, 0), False), ((2, 0), False), ((0, 0), False), ((2, 1), False), ((1, -1), False), ((-1, 2), False),
                                            ((3, 5), True), ((-1, -1), True), ((10, 10), False)])
def test_the_reference_against_a_brute_force_loop_on_3_by_7(window, causal):
  g = torch.Generator().manual_seed(3)
  sq, n, H, D = 3, 7, 2, 4
  q = torch.randn(1, sq, H, D, generator=g, dtype=torch.float64)
  kc, vc = torch.randn(1, 9, H, D, generator=g, dtype=torch.float64), torch.randn(1, 9, H, D, generator=g, dtype=torch.float64)
  o, lse, pmax, p2sum = W.attend(q, kc, vc, [n], None, window, causal)
  bo, bl = _brute(q[0], kc[0], vc[0], n, window, causal, D ** -0.5)
  torch.testing.assert_close(o[0], bo, atol=1e-12, rtol=1e-12)
  torch.testing.assert_close(lse[0], bl, atol=1e-12, rtol=1e-12)
  assert float(pmax.max()) <= 1.0 and float(p2sum.max()) <= 1.0 + 1e-12


def test_the_reference_agrees_with_kvcache_ref_where_there_is_no_window_and_marks_empty_rows():
  import kvcache_ref as R

  g = torch.Generator().manual_seed(5)
  q = torch.randn(2, 4, 4, 8, generator=g, dtype=torch.float64)
  kc, vc = torch.randn(2, 16, 2, 8, generator=g, dtype=torch.float64), torch.randn(2, 16, 2, 8, generator=g, dtype=torch.float64)
  for causal in (False, True):
    a, b = W.attend(q, kc, vc, [2, 11], None, (-1, -1), causal), R.attend(q, kc, vc, [2, 11], None, causal)
    for x, y in zip(a, b):
      torch.testing.assert_close(x, y, atol=1e-13, rtol=1e-13)
  # (-1, 0) is the causal call; rows below key 0 (L < Sq) and an empty sequence see nothing
  o, lse, _, _ = W.attend(q, kc, vc, [2, 0], None, (1, 0), False)
  assert torch.isneginf(lse[0, :, :2]).all() and torch.isfinite(lse[0, :, 2:]).all() and torch.isneginf(lse[1]).all()
  assert (o[0, :2] == 0).all() and (o[1] == 0).all()
  # pos_i + right < 0 hides a row; the tiles no row sees
  assert W.visible(4, 2, (-1, 0), False).tolist() == [[False, False], [False, False], [True, False], [True, True]]
  assert W.seen_tiles(1, 1500, (128, 0), False, 64) == {21, 22, 23}
  assert W.seen_tiles(4, 1000, (70, 0), False, 64) == {14, 15}
