"""FP8 (OCP e4m3) latent caches — ffpa_attn_with_kvcache_mla_fp8 / ffpa_attn_varlen_with_kvcache_mla_fp8 / quantize_latent_rows: what can be checked without
a GPU.  The entry points and their refusals, the fake ops, the quantisation's definition on its edge values, the C exports' argument checks and plan, and the host
replay of the FP8 build's LDS writes (tools/sim_lds_layout.py ``check_mla_fp8_writes``)."""
import ctypes
import importlib.util
import os
import subprocess

import pytest
import torch

import ffpa_attn_amd
from ffpa_attn_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALE = 192 ** -0.5
F8 = torch.float8_e4m3fn


@pytest.fixture(scope="module")
def lib():
  if not hip.library_available():
    from ffpa_attn_amd import build

    build.build()
  return hip.load_library()


# ----------------------------------------------------------------------------- the Python entries
def test_the_entry_points_are_exported():
  for name in ("ffpa_attn_with_kvcache_mla_fp8", "ffpa_attn_varlen_with_kvcache_mla_fp8", "quantize_latent_rows"):
    assert name in ffpa_attn_amd.__all__
    assert getattr(ffpa_attn_amd, name) is getattr(ffpa_attn_amd.kvcache, name)


def _args(B=2, sq=1, hq=16, hkv=1, d=576, page=64, pages=4, dtype=F8):
  q = torch.zeros(B, sq, hq, d, dtype=torch.bfloat16)
  pool = torch.zeros(B * pages, page, hkv, d, dtype=dtype)
  table = torch.arange(B * pages, dtype=torch.int32).view(B, pages)
  return q, pool, table


def _call(q, pool, table, dv=512, **kw):
  kw.setdefault("cache_seqlens", 7)
  kw.setdefault("softmax_scale", SCALE)
  return ffpa_attn_amd.ffpa_attn_with_kvcache_mla_fp8(q, pool, dv, block_table=table, **kw)


def _call_varlen(q, pool, table, dv=512, **kw):
  B = table.size(0)
  kw.setdefault("softmax_scale", SCALE)
  cu = torch.arange(B + 1, dtype=torch.int32) * (q.size(0) // B)
  return ffpa_attn_amd.ffpa_attn_varlen_with_kvcache_mla_fp8(q, pool, dv, cu, max(q.size(0) // B, 1), torch.full((B,), 7, dtype=torch.int32), table, **kw)


@pytest.mark.parametrize("dtype", [torch.float8_e4m3fnuz, torch.float8_e5m2, torch.float8_e5m2fnuz, torch.bfloat16, torch.uint8])
def test_only_ocp_e4m3_pools_are_served_and_the_message_says_so(dtype):
  q, pool, table = _args(dtype=dtype)
  with pytest.raises(TypeError, match=r"torch\.float8_e4m3fn kv_cache.*OCP e4m3 is the chip's FP8 format"):
    _call(q, pool, table)
  with pytest.raises(TypeError, match=r"OCP e4m3 is the chip's FP8 format"):
    _call_varlen(q.view(2, 16, 576), pool, table)


def test_q_and_kv_stay_16_bit():
  q, pool, table = _args()
  with pytest.raises(TypeError, match="fp16/bf16 q"):
    _call(q.float(), pool, table)
  with pytest.raises(TypeError, match="fp16/bf16 q"):
    _call(q.to(F8), pool, table)
  with pytest.raises(TypeError, match="kv must have q's dtype torch.bfloat16"):
    _call(q, pool, table, kv=torch.zeros(2, 1, 1, 576, dtype=F8))
  with pytest.raises(TypeError, match="kv must have q's dtype torch.bfloat16"):
    _call_varlen(q.view(2, 16, 576), pool, table, kv=torch.zeros(2, 1, 576, dtype=torch.float16))


@pytest.mark.parametrize("call, qshape", [(_call, (2, 1, 16, 576)), (_call_varlen, (2, 16, 576))])
def test_kv_scale_is_a_finite_positive_host_float(call, qshape):
  _, pool, table = _args()
  q = torch.zeros(qshape, dtype=torch.bfloat16)
  for bad in (torch.tensor(0.5), torch.tensor([0.5])):
    with pytest.raises(TypeError, match="kv_scale must be a host float, not a tensor.*read-back"):
      call(q, pool, table, kv_scale=bad)
  for bad in ("0.5", None, True):
    with pytest.raises(TypeError, match="kv_scale must be a real number"):
      call(q, pool, table, kv_scale=bad)
  for bad in (0.0, -1.0, float("inf"), float("nan"), 1e-320):
    with pytest.raises(ValueError, match="kv_scale must be finite and > 0"):
      call(q, pool, table, kv_scale=bad)


def test_the_latent_calls_rules_hold():
  q, pool, table = _args()
  for kw in ({}, {"softmax_scale": None}):
    with pytest.raises(TypeError, match="softmax_scale is required"):
      ffpa_attn_amd.ffpa_attn_with_kvcache_mla_fp8(q, pool, 512, cache_seqlens=7, block_table=table, **kw)
  with pytest.raises(NotImplementedError, match=r"\(576, 448\) is not built"):
    _call(q, pool, table, dv=448)
  with pytest.raises(ValueError, match="page_size .96. must be a positive multiple of 64"):
    _call(q, _args(page=128)[1][:, :96], table)
  with pytest.raises(ValueError, match="multiple of 64"):  # a contiguous cache of capacity 100
    ffpa_attn_amd.ffpa_attn_with_kvcache_mla_fp8(q, torch.zeros(2, 100, 1, 576, dtype=F8), 512, cache_seqlens=7, softmax_scale=SCALE)
  with pytest.raises(ValueError, match=r"kv must be \[B=2, Snew, Hkv=1, D=576\]"):
    _call(q, pool, table, kv=torch.zeros(2, 1, 2, 576, dtype=torch.bfloat16))
  with pytest.raises(NotImplementedError, match="inference only"):
    _call(q.clone().requires_grad_(True), pool, table)
  with pytest.raises(NotImplementedError, match="_mla_fp8_fwd_hip"):  # (no quiet fall-back on a CPU tensor: the op has a GPU kernel or nothing)
    _call(q, pool, table)


@pytest.mark.parametrize("kw", [dict(rotary_cos=torch.zeros(256, 32)), dict(window_size=(64, 0)), dict(softcap=30.0), dict(tree_mask=torch.ones(1, 1, dtype=torch.bool)),
                                dict(alibi_slopes=torch.zeros(16)), dict(k_scale=1.0)])
def test_unserved_keywords_raise_by_name(kw):
  q, pool, table = _args()
  with pytest.raises(NotImplementedError, match=f"ffpa_attn_with_kvcache_mla_fp8 does not support: {next(iter(kw))}"):
    _call(q, pool, table, **kw)
  with pytest.raises(NotImplementedError, match=f"ffpa_attn_varlen_with_kvcache_mla_fp8 does not support: {next(iter(kw))}"):
    _call_varlen(q.view(2, 16, 576), pool, table, **kw)


def test_the_16_bit_latent_calls_point_at_the_fp8_calls():
  assert "ffpa_attn_with_kvcache_mla_fp8" in ffpa_attn_amd.ffpa_attn_with_kvcache_mla.__doc__
  assert "ffpa_attn_varlen_with_kvcache_mla_fp8" in ffpa_attn_amd.ffpa_attn_varlen_with_kvcache_mla.__doc__
  q, pool, table = _args()
  with pytest.raises(TypeError, match="only supports fp16/bf16"):  # (and keep refusing such a pool themselves)
    ffpa_attn_amd.ffpa_attn_with_kvcache_mla(q, pool, 512, cache_seqlens=7, block_table=table, softmax_scale=SCALE)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_the_ops_have_fakes(dtype):
  q = torch.empty(12, 128, 576, dtype=dtype, device="meta")
  pool = torch.empty(40, 64, 1, 576, dtype=F8, device="meta")
  i32 = lambda *s: torch.empty(s, dtype=torch.int32, device="meta")
  o, lse = torch.ops.ffpa_attn._mla_fp8_fwd_hip(q, pool, 512, 0.25, i32(4), i32(3), i32(3, 8), None, None, 4, 512, 0.07, 1)
  assert o.shape == (12, 128, 512) and o.dtype == dtype and lse.shape == (128, 12) and lse.dtype == torch.float32
  kv = torch.empty(12, 1, 576, dtype=dtype, device="meta")
  used = torch.ops.ffpa_attn._mla_fp8_append_varlen_hip(pool, kv, 0.25, i32(4), i32(3), i32(3, 8))
  assert used.shape == (3,) and used.dtype == torch.int32


# ----------------------------------------------------------------------------- the quantisation
def _finite_codes():
  codes = torch.arange(256, dtype=torch.int32).to(torch.uint8)
  codes = codes[(codes & 0x7F) != 0x7F]
  assert codes.numel() == 254
  return codes


def _rne_e4m3(x: float) -> float:
  """The definition, in Python floats (exact: doubles hold every value involved): clamp to +-448, then the nearest e4m3 value, ties to the even code."""
  import math

  if math.isnan(x):
    return x
  x = max(-448.0, min(448.0, x))
  grid = sorted(set(_finite_codes().view(F8).double().abs().tolist()))  # 0, 2^-9 ... 448: code index = position
  a = abs(x)
  lo = max(i for i, g in enumerate(grid) if g <= a)
  hi = min(lo + 1, len(grid) - 1)
  if a - grid[lo] < grid[hi] - a or hi == lo:
    pick = lo
  elif a - grid[lo] > grid[hi] - a:
    pick = hi
  else:
    pick = lo if lo % 2 == 0 else hi  # (the magnitude's position IS its code: even position = even mantissa bit)
  return math.copysign(grid[pick], x)


def _edge_values():
  """+-0, +-2^-9 (the smallest subnormal), +-2^-10 (a tie to zero), mid-points between neighbouring codes (each representable in bf16), +-448, +-449 (bf16: 448),
  +-464 (half a step past the largest), +-1e4, +-inf, NaN."""
  mids = [2.0 ** -9 * 1.5, 2.0 ** -9 * 2.5, 2.0 ** -6 * 1.0625, 1.0625, 1.1875, 17.0, 19.0, 416.0 + 16.0, 0.9375 + 0.03125]
  vals = [0.0, 2.0 ** -9, 2.0 ** -10, 448.0, 449.0, 464.0, 1e4, float("inf")] + mids
  return [s * v for v in vals for s in (1.0, -1.0)] + [float("nan")]


@pytest.mark.parametrize("kv_scale", [1.0, 0.37, 4.0])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_quantize_latent_rows_on_the_edge_values(kv_scale, dtype):
  x = torch.tensor(_edge_values(), dtype=dtype)
  got = ffpa_attn_amd.quantize_latent_rows(x, kv_scale)
  assert got.dtype == F8 and got.shape == x.shape
  inv = torch.tensor(1.0 / kv_scale, dtype=torch.float32)
  scaled = (x.float() * inv).double().tolist()  # the definition's float32 product, then exact
  for xi, si, gi, code in zip(x.tolist(), scaled, got.double().tolist(), got.view(torch.uint8).tolist()):
    want = _rne_e4m3(si)
    if want != want:
      assert gi != gi and code & 0x7F == 0x7F, (xi, code)
    else:
      assert gi == want and (gi != 0 or (code == 0x80) == (str(si)[0] == "-")), (xi, si, gi, want, code)
  assert torch.isfinite(got.float()[:-1]).all()  # (+-inf and everything past +-448 saturate: no overflow turns into NaN)


def test_the_edge_table_at_scale_one_by_hand():
  x = torch.tensor([0.0, -0.0, 2.0 ** -9, -2.0 ** -9, 2.0 ** -10, -2.0 ** -10, 1.5 * 2.0 ** -9, 2.5 * 2.0 ** -9, 448.0, 464.0, 1e4, float("inf"), -float("inf"), float("nan")],
                   dtype=torch.bfloat16)
  codes = ffpa_attn_amd.quantize_latent_rows(x, 1.0).view(torch.uint8).tolist()
  assert codes[:13] == [0x00, 0x80, 0x01, 0x81, 0x00, 0x80, 0x02, 0x02, 0x7E, 0x7E, 0x7E, 0x7E, 0xFE] and codes[13] & 0x7F == 0x7F
  # torch's bare conversion is NOT the definition: it turns overflow into NaN
  assert torch.tensor([1e4]).to(F8).float().isnan().all()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_every_finite_code_survives_the_round_trip(dtype):
  codes = _finite_codes()
  wide = codes.view(F8).to(dtype)
  assert (wide.double() == codes.view(F8).double()).all()  # every e4m3 value is exactly a bf16 / an fp16: what the kernel's widening rests on
  back = ffpa_attn_amd.quantize_latent_rows(wide, 1.0)
  assert (back.view(torch.uint8) == codes).all()
  for s in (0.25, 8.0):  # a power-of-two scale is exact as well
    assert (ffpa_attn_amd.quantize_latent_rows(wide * s, s).view(torch.uint8) == codes).all()


def test_quantize_latent_rows_refuses_what_it_cannot_mean():
  with pytest.raises(TypeError, match="floating-point tensor"):
    ffpa_attn_amd.quantize_latent_rows(torch.zeros(4, dtype=torch.int32), 1.0)
  with pytest.raises(ValueError, match="finite and > 0"):
    ffpa_attn_amd.quantize_latent_rows(torch.zeros(4), 0.0)
  with pytest.raises(TypeError, match="not a tensor"):
    ffpa_attn_amd.quantize_latent_rows(torch.zeros(4), torch.tensor(1.0))


# ----------------------------------------------------------------------------- the C ABI
FP8_SYMBOLS = ("ffpa_attn_varlen_mla_fp8_fwd", "ffpa_attn_varlen_mla_fp8_fwd_plan", "ffpa_attn_varlen_mla_fp8_fwd_kernel", "ffpa_attn_varlen_mla_fp8_fwd_workspace_bytes",
               "ffpa_attn_varlen_mla_fp8_fwd_compact_slots", "ffpa_attn_mla_fp8_append_varlen")


def test_abi_version_stays_7_and_the_symbols_are_exported(lib):
  assert hip.ABI_VERSION == 7 and lib.ffpa_attn_query(0) == 7
  for name in FP8_SYMBOLS:
    assert name in hip.EXPORTS and getattr(lib, name) is not None, name


def test_ctypes_mirror_of_ffpa_mla_fp8_matches_the_c_header(tmp_path):
  fields = [f[0] for f in hip.FfpaMlaFp8._fields_]
  src = tmp_path / "layout.c"
  body = "".join(f'printf("{f} %zu\\n", offsetof(ffpa_mla_fp8, {f}));\n' for f in fields)
  src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ffpa_attn.h"\nint main(void){\nprintf("sizeof %zu\\n", sizeof(ffpa_mla_fp8));\n'
                 'printf("mla %zu\\n", sizeof(ffpa_mla));\nprintf("append %zu\\n", sizeof(ffpa_mla_append_varlen_params));\n' + body + "return 0;}\n")
  exe = tmp_path / "layout"
  subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
  out = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
  assert int(out["sizeof"]) == ctypes.sizeof(hip.FfpaMlaFp8) == 16
  assert fields == ["struct_size", "reserved", "kv_scale", "reserved2"]
  for f in fields:
    assert int(out[f]) == getattr(hip.FfpaMlaFp8, f).offset, f
  assert int(out["mla"]) == ctypes.sizeof(hip.FfpaMla) == 56 and int(out["append"]) == ctypes.sizeof(hip.FfpaMlaAppendVarlenParams)  # (the structs it rides with keep their layout)


_KEEP = []


def _buf():
  buf = (ctypes.c_char * 4096)()
  _KEEP.append(buf)
  return (ctypes.addressof(buf) + 15) & ~15


def _call_args(d=576, dv=512, sq=1, B=32, hq=128, hkv=1, max_k=4096, causal=False, num_splits=0, flags=0, total_q=None, over=None, f8_over=None, no_f8=False,
               row_stride=None, page_stride=None, kv_scale=0.5):
  """A well-formed FP8 latent call on host buffers (only the argument checks and the plan run on it) -> the ctypes arguments (p, kv, m, f8 | None) + their owners."""
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
  m = hip._stamped(hip.FfpaMla)
  m.head_dim_v = dv
  f8 = hip._stamped(hip.FfpaMlaFp8)
  f8.kv_scale = kv_scale
  for k_, v_ in (f8_over or {}).items():
    setattr(f8, k_, v_)
  return ctypes.byref(p), ctypes.byref(kv), ctypes.byref(m), (None if no_f8 else ctypes.byref(f8)), (p, kv, m, f8)


@pytest.mark.parametrize("kw, status, text", [
  (dict(no_f8=True), 1, b"mla_fp8 is NULL"),
  (dict(f8_over=dict(struct_size=8)), 10, b"ffpa_mla_fp8 ABI mismatch"),
  (dict(f8_over=dict(struct_size=0)), 10, b"ffpa_mla_fp8 ABI mismatch"),
  (dict(f8_over=dict(reserved=1)), 10, b"ffpa_mla_fp8.reserved"),
  (dict(f8_over=dict(reserved2=1.0)), 10, b"reserved2"),
  (dict(kv_scale=0.0), 4, b"ffpa_mla_fp8.kv_scale"),
  (dict(kv_scale=-0.5), 4, b"kv_scale=-0.5 must be finite and > 0"),
  (dict(kv_scale=float("inf")), 4, b"ffpa_mla_fp8.kv_scale"),
  (dict(kv_scale=float("nan")), 4, b"ffpa_mla_fp8.kv_scale"),
  (dict(row_stride=576 + 8), 5, b"multiples of 16 elements"),
  (dict(page_stride=64 * 576 + 8), 5, b"multiples of 16 elements"),
  # the latent call's own refusals stay what they are
  (dict(dv=576), 3, b"(576, 576) is not built"),
  (dict(over=dict(dtype=2)), 2, b"dtype"),
  (dict(over=dict(abi_version=6)), 10, b"ffpa_varlen_fwd_params ABI mismatch"),
])
def test_status_codes_of_the_c_call_come_before_any_device_work(lib, kw, status, text):
  p, kv, m, f8, keep = _call_args(**kw)
  for fn, extra in ((lib.ffpa_attn_varlen_mla_fp8_fwd, (None,)), (lib.ffpa_attn_varlen_mla_fp8_fwd_plan, ((ctypes.c_int * 5)(),)),
                    (lib.ffpa_attn_varlen_mla_fp8_fwd_kernel, (ctypes.create_string_buffer(200), 200)),
                    (lib.ffpa_attn_varlen_mla_fp8_fwd_compact_slots, (ctypes.byref(ctypes.c_int(0)),))):
    assert fn(p, kv, m, f8, *extra) == status, fn
    assert text in lib.ffpa_attn_last_error(), lib.ffpa_attn_last_error()
  assert lib.ffpa_attn_varlen_mla_fp8_fwd_workspace_bytes(p, kv, m, f8) == 0


@pytest.mark.parametrize("f8_over, no_f8, status, text", [
  (None, True, 1, b"mla_fp8 is NULL"),
  (dict(struct_size=12), False, 10, b"ffpa_mla_fp8 ABI mismatch"),
  (dict(reserved=7), False, 10, b"ffpa_mla_fp8.reserved"),
  (dict(kv_scale=0.0), False, 4, b"ffpa_mla_fp8.kv_scale"),
])
def test_the_ragged_append_refuses_a_bad_struct_first(lib, f8_over, no_f8, status, text):
  f8 = hip._stamped(hip.FfpaMlaFp8)
  f8.kv_scale = 1.0
  for k_, v_ in (f8_over or {}).items():
    setattr(f8, k_, v_)
  assert lib.ffpa_attn_mla_fp8_append_varlen(None, None, None if no_f8 else ctypes.byref(f8), None) == status
  assert text in lib.ffpa_attn_last_error(), lib.ffpa_attn_last_error()
  assert lib.ffpa_attn_mla_fp8_append_varlen(None, None, ctypes.byref(hip._stamped(hip.FfpaMlaFp8)), None) == 4  # (a zeroed scale)
  ok = hip._stamped(hip.FfpaMlaFp8)
  ok.kv_scale = 2.0
  assert lib.ffpa_attn_mla_fp8_append_varlen(None, None, ctypes.byref(ok), None) == 1 and b"params is NULL" in lib.ffpa_attn_last_error()


PLAN_SHAPES = [dict(B=32, hq=16, sq=1, max_k=1024), dict(B=32, hq=128, sq=1, max_k=4096), dict(B=32, hq=128, sq=4, max_k=4096, causal=True),
               dict(B=4, hq=16, sq=1, max_k=16384), dict(B=6, hq=128, sq=40, total_q=45, max_k=4096), dict(B=2, hq=32, hkv=2, sq=3, max_k=300, num_splits=3, flags=hip.FLAG_FORCE_SPLITS)]


@pytest.mark.parametrize("shape", PLAN_SHAPES)
def test_the_plan_is_the_latent_calls(lib, shape, monkeypatch):
  """Same shapes, no forced stream flag, caches far below the non-temporal rule's 272 MiB: the plan (row tiles, block rows, tile keys, grid, KV ranges), the scratch
  and the compact grid of the FP8 call are those of the 16-bit latent call."""
  monkeypatch.setenv("FFPA_HIP_FAKE_CUS", "256")
  p, kv, m, f8, keep = _call_args(**shape)
  got, want = (ctypes.c_int * 5)(), (ctypes.c_int * 5)()
  assert lib.ffpa_attn_varlen_mla_fp8_fwd_plan(p, kv, m, f8, got) == 0, lib.ffpa_attn_last_error()
  assert lib.ffpa_attn_varlen_mla_fwd_plan(p, kv, m, want) == 0, lib.ffpa_attn_last_error()
  assert list(got) == list(want)
  assert lib.ffpa_attn_varlen_mla_fp8_fwd_workspace_bytes(p, kv, m, f8) == lib.ffpa_attn_varlen_mla_fwd_workspace_bytes(p, kv, m)
  s8, s16 = ctypes.c_int(-1), ctypes.c_int(-1)
  assert lib.ffpa_attn_varlen_mla_fp8_fwd_compact_slots(p, kv, m, f8, ctypes.byref(s8)) == 0 and lib.ffpa_attn_varlen_mla_fwd_compact_slots(p, kv, m, ctypes.byref(s16)) == 0
  assert s8.value == s16.value
  name8, name16 = ctypes.create_string_buffer(256), ctypes.create_string_buffer(256)
  assert lib.ffpa_attn_varlen_mla_fp8_fwd_kernel(p, kv, m, f8, name8, 256) == 0 and lib.ffpa_attn_varlen_mla_fwd_kernel(p, kv, m, name16, 256) == 0
  assert name8.value.startswith(b"ffpa_fwd_m16_mla_fp8_kernel<bf16, 576, dv=512")
  assert name8.value == name16.value.replace(b"ffpa_fwd_m16_mla_kernel", b"ffpa_fwd_m16_mla_fp8_kernel")


def test_the_non_temporal_rule_sees_half_the_bytes(lib, monkeypatch):
  """One reader per byte, B x max_seqlen_kv x 576 elements: 272 MiB of bf16 is 136 MiB of e4m3 — the 16-bit call takes the NT build, the FP8 call on the same
  shape does not; at twice the keys both do."""
  monkeypatch.setenv("FFPA_HIP_FAKE_CUS", "256")
  keys = -(-(272 << 20) // (32 * 576 * 2) // 64) * 64
  names = {}
  for mult in (1, 2):
    p, kv, m, f8, keep = _call_args(B=32, hq=16, sq=1, max_k=keys * mult)
    n8, n16 = ctypes.create_string_buffer(256), ctypes.create_string_buffer(256)
    assert lib.ffpa_attn_varlen_mla_fp8_fwd_kernel(p, kv, m, f8, n8, 256) == 0 and lib.ffpa_attn_varlen_mla_fwd_kernel(p, kv, m, n16, 256) == 0
    names[mult] = (b", NT>" in n8.value, b", NT>" in n16.value)
  assert names == {1: (False, True), 2: (True, True)}


# ----------------------------------------------------------------------------- the LDS image of the FP8 build
def test_the_fp8_builds_lds_writes_leave_the_dma_image_and_are_conflict_free():
  spec = importlib.util.spec_from_file_location("sim_lds_layout", os.path.join(ROOT, "tools", "sim_lds_layout.py"))
  sim = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(sim)
  assert sim.check_mla_fp8_writes(576, quiet=True) == (1, 0)  # lane-linear 16-byte stores: 8 lanes x 4 dwords = the 32 banks, once
  # the replay is not vacuous: with another map the image is still the DMA's (both builds swizzle the SOURCE), without the lane-linear rule it would not be free
  assert sim.check_mla_fp8_writes(576, sim.m16_k_sw, quiet=True) == (1, 0)
  assert sim.check_m16_shared(576, quiet=True) == (1, 1, 0, 0)  # (the reads of that image: tests/test_mla_lds_layout.py)
