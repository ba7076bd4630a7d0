"""The soft-capping entry point without a GPU: the export and its argument errors, the refusals of ffpa_attn_varlen_softcap_fwd (they come before any device
work), the kernel names, the plan — the window call's for the same (p, kv, w) —, the float64 reference (tests/kvcache_softcap_ref.py) against a brute-force
loop, and the kernel's tanh formula in float32 against float64 ``tanh``."""

import ctypes
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ffpa_attn_amd
import kvcache_softcap_ref as S
import kvcache_window_ref as W
from ffpa_attn_amd import (ffpa_attn_func, ffpa_attn_varlen_func, ffpa_attn_with_kvcache, ffpa_attn_with_kvcache_softcap, ffpa_attn_with_kvcache_window, hip)
from test_kvcache_window import _call_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
  if not hip.library_available():
    from ffpa_attn_amd import build

    build.build()
  return hip.load_library()


# ----------------------------------------------------------------------------- the Python entry
def test_the_entry_point_is_exported():
  assert "ffpa_attn_with_kvcache_softcap" in ffpa_attn_amd.__all__
  assert ffpa_attn_amd.ffpa_attn_with_kvcache_softcap is ffpa_attn_with_kvcache_softcap


def _cpu_args(B=2, sq=1, hq=8, hkv=2, d=128, cap=256):
  q = torch.zeros(B, sq, hq, d, dtype=torch.bfloat16)
  kc = torch.zeros(B, cap, hkv, d, dtype=torch.bfloat16)
  return q, kc, kc.clone()


def test_softcap_is_required_and_checked():
  q, kc, vc = _cpu_args()
  with pytest.raises(TypeError):
    ffpa_attn_with_kvcache_softcap(q, kc, vc, cache_seqlens=7)  # (keyword-only, no default)
  for bad in (None, "30", True, False, (30.0,), [50], torch.tensor(30.0), 30j):
    with pytest.raises(TypeError, match="softcap must be a real number"):
      ffpa_attn_with_kvcache_softcap(q, kc, vc, cache_seqlens=7, softcap=bad)
  for bad in (-1, -30.0, -0.001, float("nan"), float("inf"), float("-inf")):
    with pytest.raises(ValueError, match="softcap"):
      ffpa_attn_with_kvcache_softcap(q, kc, vc, cache_seqlens=7, softcap=bad)


def test_window_size_errors_are_the_window_calls():
  q, kc, vc = _cpu_args()
  for bad in (None, 64, (64,), (1, 2, 3), "ab", (64, 2.0), (True, 0)):
    with pytest.raises(TypeError) as win:
      ffpa_attn_with_kvcache_window(q, kc, vc, cache_seqlens=7, window_size=bad)
    for cap in (30.0, 0):
      with pytest.raises(TypeError) as got:
        ffpa_attn_with_kvcache_softcap(q, kc, vc, cache_seqlens=7, softcap=cap, window_size=bad)
      assert str(got.value) == str(win.value)
  for bad in ((-2, 0), (0, -2)):
    with pytest.raises(ValueError) as win:
      ffpa_attn_with_kvcache_window(q, kc, vc, cache_seqlens=7, window_size=bad)
    with pytest.raises(ValueError) as got:
      ffpa_attn_with_kvcache_softcap(q, kc, vc, cache_seqlens=7, softcap=50, window_size=bad)
    assert str(got.value) == str(win.value)


def test_what_the_window_call_refuses_is_refused_with_the_same_text():
  q, kc, vc = _cpu_args()
  knew = torch.zeros(2, 1, 2, 128, dtype=torch.bfloat16)
  for args, kw in (((q.float(), kc, vc), {}), ((q, kc, vc[:, :100]), {}), ((q[0], kc, vc), {}), ((q[:, :, :3], kc, vc), {}), ((q, kc, vc), dict(num_splits=-1)),
                   ((q, kc, vc), dict(cache_seqlens=-4)), ((q, kc, vc), dict(cache_seqlens="7")), ((q, kc, vc), dict(block_table=torch.zeros(2, 4, dtype=torch.int64))),
                   ((q, kc, vc), dict(k=knew, cache_seqlens=3)), ((q, kc, vc), dict(rotary_cos=torch.zeros(256, 8, dtype=torch.bfloat16), cache_seqlens=3)),
                   ((q, kc, vc), dict(k=knew, v=knew)), ((q, kc, vc), dict(k=knew, v=knew[:, :, :1], cache_seqlens=3))):
    with pytest.raises(Exception) as win:
      ffpa_attn_with_kvcache_window(*args, **kw, window_size=(64, 0))
    with pytest.raises(type(win.value)) as got:
      ffpa_attn_with_kvcache_softcap(*args, **kw, window_size=(64, 0), softcap=30.0)
    assert str(got.value) == str(win.value)


def test_a_tensor_that_requires_grad_raises():
  q, kc, vc = _cpu_args()
  for i in range(3):
    args = [q, kc, vc]
    args[i] = args[i].clone().requires_grad_(True)
    for kw in (dict(softcap=30.0), dict(softcap=50.0, window_size=(64, 0)), dict(softcap=0)):
      with pytest.raises(NotImplementedError, match="inference only"):
        ffpa_attn_with_kvcache_softcap(*args, cache_seqlens=7, **kw)


def test_the_existing_entries_keep_refusing_softcap():
  q, kc, vc = _cpu_args()
  with pytest.raises(NotImplementedError, match="softcap"):
    ffpa_attn_with_kvcache(q, kc, vc, cache_seqlens=7, softcap=30.0)
  with pytest.raises(TypeError):
    ffpa_attn_with_kvcache_window(q, kc, vc, cache_seqlens=7, window_size=(64, 0), softcap=30.0)
  import inspect

  for fn in (ffpa_attn_func, ffpa_attn_amd.ffpa_attn_with_kvcache_tree, ffpa_attn_amd.ffpa_attn_with_kvcache_window):
    assert "softcap" not in inspect.signature(fn).parameters, fn
  assert ffpa_attn_varlen_func is ffpa_attn_amd.ffpa_attn_varlen_func


def test_the_op_has_a_fake_shaped_like_the_window_ops():
  names = [a.name for a in torch.ops.ffpa_attn._softcap_fwd_hip.default._schema.arguments]
  assert names == ["q", "k", "v", "cu_seqlens_q", "cu_seqlens_k", "seqused_k", "block_table", "softcap", "window_left", "window_right", "max_seqlen_q",
                   "max_seqlen_k", "softmax_scale", "causal", "rescale_threshold", "num_splits"]
  q = torch.empty(12, 8, 128, dtype=torch.bfloat16, device="meta")
  kv = torch.empty(40, 64, 2, 128, dtype=torch.bfloat16, device="meta")
  i32 = lambda *s: torch.empty(s, dtype=torch.int32, device="meta")
  o, lse = torch.ops.ffpa_attn._softcap_fwd_hip(q, kv, kv, i32(4), None, i32(3), i32(3, 8), 50.0, 64, 0, 4, 512, 0.1, 1)
  assert o.shape == (12, 8, 128) and o.dtype == torch.bfloat16 and lse.shape == (8, 12) and lse.dtype == torch.float32


def test_the_op_level_call_checks_softcap_before_the_device():
  q = torch.zeros(4, 8, 128, dtype=torch.bfloat16)
  for bad, exc in ((True, TypeError), ("30", TypeError), (-1.0, ValueError), (0.0, ValueError), (float("nan"), ValueError), (float("inf"), ValueError)):
    with pytest.raises(exc, match="softcap"):
      hip.softcap_forward(q, q, q, None, None, 1, 64, False, 0.1, bad)
  with pytest.raises(NotImplementedError, match="_softcap_fwd_hip"):  # (a CPU tensor: the kernel needs a GPU tensor)
    hip.softcap_forward(q, q, q, None, None, 1, 64, False, 0.1, 30.0)


# ----------------------------------------------------------------------------- the C ABI
SOFTCAP_SYMBOLS = ("ffpa_attn_varlen_softcap_fwd", "ffpa_attn_varlen_softcap_fwd_plan", "ffpa_attn_varlen_softcap_fwd_kernel",
                   "ffpa_attn_varlen_softcap_fwd_workspace_bytes")


def test_abi_version_stays_7_and_the_four_symbols_are_exported(lib):
  assert hip.ABI_VERSION == 7 and lib.ffpa_attn_query(0) == 7
  for name in SOFTCAP_SYMBOLS:
    assert name in hip.EXPORTS and getattr(lib, name) is not None, name
  header = open(os.path.join(ROOT, "include", "ffpa_attn.h")).read()
  declared = set(re.findall(r"^\s*(?:int|size_t|const char\*)\s+(ffpa_attn_\w+)\s*\(", header, flags=re.M))
  assert declared == set(hip.EXPORTS)


def _each(lib, p, kv, w, cap):
  """The launch, the plan and the kernel query on one set of arguments -> their statuses (and the workspace query's answer)."""
  c = ctypes.c_float(cap)
  yield lib.ffpa_attn_varlen_softcap_fwd(p, kv, w, c, None)
  yield lib.ffpa_attn_varlen_softcap_fwd_plan(p, kv, w, c, (ctypes.c_int * 5)())
  yield lib.ffpa_attn_varlen_softcap_fwd_kernel(p, kv, w, c, ctypes.create_string_buffer(200), 200)


@pytest.mark.parametrize("paged", [True, False])
@pytest.mark.parametrize("cap", [0.0, -0.0, -30.0, float("nan"), float("inf"), float("-inf")])
def test_a_bad_softcap_returns_a_status_before_any_device_work(lib, paged, cap):
  p, kv, w, keep = _call_args(paged=paged)
  for w_ in (w, None):
    for rc in _each(lib, p, kv, w_, cap):
      assert rc == 4 and b"softcap" in lib.ffpa_attn_last_error(), lib.ffpa_attn_last_error()
    assert lib.ffpa_attn_varlen_softcap_fwd_workspace_bytes(p, kv, w_, ctypes.c_float(cap)) == 0


@pytest.mark.parametrize("paged", [True, False])
@pytest.mark.parametrize("kw, status, text", [
  (dict(win_over=dict(struct_size=12)), 10, b"ffpa_window ABI mismatch"),
  (dict(win_over=dict(reserved=1)), 10, b"reserved"),
  (dict(window=(-2, 0)), 4, b"must be >= -1"),
  # the packed call's own refusals come first
  (dict(over=dict(dtype=2)), 2, b"dtype"),
  (dict(over=dict(head_dim=1032)), 3, b"headdim not support"),
  (dict(over=dict(abi_version=6)), 10, b"ffpa_varlen_fwd_params ABI mismatch"),
])
def test_every_other_check_is_the_window_calls(lib, paged, kw, status, text):
  p, kv, w, keep = _call_args(paged=paged, **kw)
  for rc in _each(lib, p, kv, w, 50.0):
    assert rc == status and text in lib.ffpa_attn_last_error(), lib.ffpa_attn_last_error()
  assert lib.ffpa_attn_varlen_softcap_fwd_workspace_bytes(p, kv, w, ctypes.c_float(50.0)) == 0


def test_a_null_p_returns_a_status(lib):
  _, kv, w, keep = _call_args(paged=True)
  for rc in _each(lib, None, kv, w, 30.0):
    assert rc == 1, lib.ffpa_attn_last_error()
  assert lib.ffpa_attn_varlen_softcap_fwd_workspace_bytes(None, kv, w, ctypes.c_float(30.0)) == 0


@pytest.mark.parametrize("paged", [True, False])
@pytest.mark.parametrize("d", [128, 512, 1024])
def test_the_kernel_name(lib, paged, d, monkeypatch):
  monkeypatch.setenv("FFPA_HIP_FAKE_CUS", "256")
  for no_window in (False, True):
    p, kv, w, keep = _call_args(paged=paged, d=d, hq=16, hkv=4, B=4, max_k=4096, no_window=no_window)
    name = ctypes.create_string_buffer(200)
    assert lib.ffpa_attn_varlen_softcap_fwd_kernel(p, kv, w, ctypes.c_float(50.0), name, 200) == 0, lib.ffpa_attn_last_error()
    assert name.value.decode().startswith(f"ffpa_fwd_m16_{'paged' if paged else 'varlen'}_softcap_kernel<bf16, {d}"), name.value
  # ... and through the Python plan query
  plan = hip.varlen_launch_plan(4, 16, 4, 1, 4096, d, total_q=4, page_size=64 if paged else 0, softcap=30.0, window=(1024, 0))
  assert f"_softcap_kernel<bf16, {d}" in plan["kernel"] and "(GQA heads packed into rows)" in plan["kernel"]


PLAN_CASES = {
  "decode": dict(B=32, hq=32, hkv=8, sq=1, max_k=32768),
  "packed rows": dict(B=3, hq=8, hkv=2, sq=4, max_k=1088),
  "chunk": dict(B=1, hq=4, hkv=2, sq=200, max_k=768),
  "forced splits": dict(B=1, hq=8, hkv=2, sq=1, max_k=1536, num_splits=5, over=dict(flags=hip.FLAG_FORCE_SPLITS)),
}


@pytest.mark.parametrize("paged", [True, False])
@pytest.mark.parametrize("d", [512, 1024])
@pytest.mark.parametrize("case", sorted(PLAN_CASES))
@pytest.mark.parametrize("window", [(4096, 0), (100, 0), (48, 16), None])
def test_the_plan_is_the_window_calls(lib, paged, d, case, window, monkeypatch):
  """Row tiles, rows, keys per tile, workgroups and splits equal ffpa_attn_varlen_window_fwd_plan's on the same params; a NULL window is (-1, -1); the workspace
  and the kernel name (but for the family) agree as well."""
  monkeypatch.setenv("FFPA_HIP_FAKE_CUS", "256")
  for causal in (True, False):
    p, kv, w, keep = _call_args(paged=paged, d=d, causal=causal, window=window or (-1, -1), **PLAN_CASES[case])
    ws = None if window is None else w
    got, want = (ctypes.c_int * 5)(), (ctypes.c_int * 5)()
    assert lib.ffpa_attn_varlen_softcap_fwd_plan(p, kv, ws, ctypes.c_float(30.0), got) == 0, lib.ffpa_attn_last_error()
    assert lib.ffpa_attn_varlen_window_fwd_plan(p, kv, w, want) == 0
    assert list(got) == list(want), (case, window, causal)
    if case == "forced splits" and window in (None, (4096, 0)):  # (a 100-key window is two KV tiles, (48, 16) one: fewer tiles than ranges)
      assert got[4] == 5
    assert lib.ffpa_attn_varlen_softcap_fwd_workspace_bytes(p, kv, ws, ctypes.c_float(30.0)) == lib.ffpa_attn_varlen_window_fwd_workspace_bytes(p, kv, w)
    a, b = ctypes.create_string_buffer(200), ctypes.create_string_buffer(200)
    assert lib.ffpa_attn_varlen_softcap_fwd_kernel(p, kv, ws, ctypes.c_float(30.0), a, 200) == 0 and lib.ffpa_attn_varlen_window_fwd_kernel(p, kv, w, b, 200) == 0
    assert a.value.decode() == b.value.decode().replace("_window_kernel<", "_softcap_kernel<")


# ----------------------------------------------------------------------------- the float64 reference
def _brute(q, k, v, n, window, causal, scale, cap):
  """Capped softmax attention of one sequence, element by element: q [sq, H, D], k / v [n, H, D] (MHA), python floats."""
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
        s = cap * math.tanh(sum(float(q[i, h, e]) * float(k[j, h, e]) for e in range(D)) * scale / cap)  # the cap on every score ...
        if (left < 0 or j >= pos - left) and (right < 0 or j <= pos + right):                            # ... the mask behind it
          scores[j] = s
      if not scores:
        continue
      m = max(scores.values())
      l = sum(math.exp(s - m) for s in scores.values())
      lse[h][i] = m + math.log(l)
      for e in range(D):
        o[i][h][e] = sum(math.exp(s - m) / l * float(v[j, h, e]) for j, s in scores.items())
  return torch.tensor(o, dtype=torch.float64), torch.tensor(lse, dtype=torch.float64)


@pytest.mark.parametrize("window, causal", [((-1, -1), False), ((-1, 0), False), ((2, 0), False), ((2, 1), False), ((3, 5), True)])
@pytest.mark.parametrize("cap", [30.0, 50.0, 2.0])
def test_the_reference_against_a_brute_force_loop_on_two_sequences(window, causal, cap):
  g = torch.Generator().manual_seed(11)
  sq, H, D, lens = 3, 2, 4, [7, 2]
  q = torch.randn(2, sq, H, D, generator=g, dtype=torch.float64) * 40  # (scores of several caps: the tanh bends them)
  kc, vc = torch.randn(2, 9, H, D, generator=g, dtype=torch.float64), torch.randn(2, 9, H, D, generator=g, dtype=torch.float64)
  o, lse, pmax, p2sum = S.attend(q, kc, vc, lens, None, window, causal, softcap=cap)
  for b, n in enumerate(lens):
    bo, bl = _brute(q[b], kc[b], vc[b], n, window, causal, D ** -0.5, cap)
    torch.testing.assert_close(o[b], bo, atol=1e-12, rtol=1e-12)
    torch.testing.assert_close(lse[b], bl, atol=1e-12, rtol=1e-12)
  assert float(pmax.max()) <= 1.0 and float(p2sum.max()) <= 1.0 + 1e-12
  # the cap matters on these scores, and "off" is the window reference
  off = S.attend(q, kc, vc, lens, None, window, causal, softcap=0.0)
  for x, y in zip(off, W.attend(q, kc, vc, lens, None, window, causal)):
    assert torch.equal(x, y)
  assert (off[0] - o).abs().max() > 1e-2


# ----------------------------------------------------------------------------- the tanh formula
def test_the_tanh_formula_in_float32_is_within_2_to_the_minus_21_of_float64_tanh():
  """``S.tanh_f32`` restates the kernel's chain operation by operation (csrc/ffpa_fwd_m16_kernel.h ``m16_softcap_tanh``).  Budget, in units of 2^-24: the
  exponent's rounding and exp2's 1 ulp reach t through 2e / (1 + e)^2 <= 1/2, the sum's rounding and the reciprocal's 1 ulp through 2 / (1 + e) <= 2, plus the
  last rounding: under 8 = 2^-21.  This holds the FORMULA (numpy's exp2 and division here); the kernel's v_exp_f32 / v_rcp_f32 are held by the GPU tests."""
  grid = np.concatenate([
    np.linspace(-20.0, 20.0, 400001),                                       # |y| <= 20
    np.array([0.0, -0.0]), np.geomspace(1e-12, 1e-4, 2001), -np.geomspace(1e-12, 1e-4, 2001),  # |y| < 1e-4
    np.geomspace(20.0, 3e38, 2001), -np.geomspace(20.0, 3e38, 2001),        # the saturated ends, up to the largest finite float32
    np.array([np.finfo(np.float32).max, -np.finfo(np.float32).max, 44.0, -44.0, 44.4, -44.4, 51.7, -51.7, 9.01, -9.01]),
  ]).astype(np.float32)
  got = S.tanh_f32(grid).astype(np.float64)
  want = np.tanh(grid.astype(np.float64))
  err = np.abs(got - want)
  print(f"[softcap] tanh formula: max abs err {err.max():.3e} = 2^{np.log2(err.max()):.2f} at y = {grid[np.argmax(err)]!r}")
  assert np.isfinite(got).all()
  assert err.max() <= 2.0 ** -21
  # exact at both saturations and at 0, and odd to within the bound
  assert S.tanh_f32(np.float32(1e30)) == 1.0 and S.tanh_f32(np.float32(-1e30)) == -1.0 and S.tanh_f32(np.float32(0.0)) == 0.0
  assert S.tanh_f32(np.float32(60.0)) == 1.0 and S.tanh_f32(np.float32(-60.0)) == -1.0
