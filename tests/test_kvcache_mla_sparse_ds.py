"""The 656-byte FP8 latent rows of DeepSeek-V3.2 without a GPU: the format (``pack_latent_rows_ds`` / ``unpack_latent_rows_ds`` against plain-Python arithmetic),
every refusal of ``ffpa_attn_with_kvcache_mla_sparse_ds`` and ``store_latent_rows_ds`` in front of a launch, the C ABI of ``ffpa_attn_varlen_mla_sparse_ds_fwd`` /
``ffpa_attn_mla_ds_store`` (statuses, their order, the plan) and the ops' fakes."""

import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import ffpa_attn_amd
from ffpa_attn_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALE = 192 ** -0.5
ROW = 656
NAMES = ("ffpa_attn_with_kvcache_mla_sparse_ds", "store_latent_rows_ds", "pack_latent_rows_ds", "unpack_latent_rows_ds")
CALL = "ffpa_attn_with_kvcache_mla_sparse_ds"


@pytest.fixture(scope="module")
def lib():
  if not hip.library_available():
    from ffpa_attn_amd import build

    build.build()
  return hip.load_library()


def test_the_four_names_are_exported():
  for name in NAMES:
    assert name in ffpa_attn_amd.__all__
    assert getattr(ffpa_attn_amd, name) is getattr(ffpa_attn_amd.kvcache, name)


# ----------------------------------------------------------------------------- the format
def _e4m3_value(code: int) -> float:
  """OCP e4m3 (bias 7, no infinities, S.1111.111 = NaN) -> float."""
  sign, e, m = -1.0 if code & 0x80 else 1.0, (code >> 3) & 15, code & 7
  if e == 15 and m == 7:
    return math.nan
  return sign * (m / 8 * 2.0 ** -6 if e == 0 else (1 + m / 8) * 2.0 ** (e - 7))


def _e4m3_code(v: float) -> int:
  """rne_e4m3 of a value in [-448, 448] (or NaN), in exact float64 arithmetic: round() is round-half-even."""
  if math.isnan(v):
    return 0x7F
  sign = 0x80 if math.copysign(1.0, v) < 0 else 0
  a = abs(v)
  if a < 2.0 ** -6:
    return sign | round(a * 2.0 ** 9)  # (subnormals in units of 2^-9; 8 units are the smallest normal, code 0x08)
  e = math.frexp(a)[1] - 1
  m = round((a / 2.0 ** e - 1) * 8)
  if m == 8:
    e, m = e + 1, 0
  return sign | ((e + 7) << 3) | m


def _bf16_rne_bits(x32: np.ndarray) -> np.ndarray:
  bits = x32.astype(np.float32).view(np.uint32).astype(np.uint64)
  return ((bits + 0x7FFF + ((bits >> 16) & 1)) >> 16).astype(np.uint16)


def _pack_reference(row: torch.Tensor) -> bytes:
  """``pack_latent_rows_ds`` of ONE row [576], restated element by element: numpy float32 scalars divide correctly rounded."""
  x = row.to(torch.float32).numpy()
  out = bytearray()
  scales = []
  for j in range(4):
    tile = x[128 * j:128 * (j + 1)]
    a = np.float32(max([abs(v) for v in tile if math.isfinite(v)] + [0.0]))
    s = max(a / np.float32(448), np.float32(2.0 ** -100))
    assert s.dtype == np.float32
    scales.append(s)
    for v in tile:
      with np.errstate(all="ignore"):
        r = float(np.float32(v) / s)
      out.append((0xFF if math.copysign(1.0, v) < 0 else 0x7F) if math.isnan(v) else _e4m3_code(min(max(r, -448.0), 448.0)))  # (NaN keeps x's sign)
  out += np.array(scales, dtype="<f4").tobytes()
  out += row[512:].to(torch.bfloat16).view(torch.int16).numpy().astype("<i2").tobytes()
  return bytes(out)


def test_the_byte_offsets_of_the_three_fields():
  kv = torch.zeros(2, 3, 576, dtype=torch.bfloat16)
  kv[..., :512] = 448.0  # scale 1, code 0x7E
  kv[..., 128:256] = 2 * 448.0  # scale 2
  kv[..., 512:] = 1.0  # bf16 0x3F80
  rows = ffpa_attn_amd.pack_latent_rows_ds(kv)
  assert rows.shape == (2, 3, ROW) and rows.dtype == torch.uint8
  assert (rows[..., :512] == 0x7E).all()
  assert rows[0, 0, 512:528].numpy().tobytes() == np.array([1, 2, 1, 1], dtype="<f4").tobytes()
  assert rows[0, 0, 528:].numpy().tobytes() == b"\x80\x3f" * 64
  for dt in (torch.float16, torch.float32):
    assert torch.equal(ffpa_attn_amd.pack_latent_rows_ds(kv.to(dt)), rows)
  back = ffpa_attn_amd.unpack_latent_rows_ds(rows)
  assert back.shape == (2, 3, 576) and back.dtype == torch.bfloat16 and torch.equal(back, kv)
  with pytest.raises(ValueError, match=r"\[\.\.\., 576\]"):
    ffpa_attn_amd.pack_latent_rows_ds(torch.zeros(4, 512, dtype=torch.bfloat16))
  with pytest.raises(TypeError, match="bf16 / fp16 / fp32"):
    ffpa_attn_amd.pack_latent_rows_ds(torch.zeros(4, 576, dtype=torch.float64))
  with pytest.raises(ValueError, match=r"\[\.\.\., 656\]"):
    ffpa_attn_amd.unpack_latent_rows_ds(torch.zeros(4, 576, dtype=torch.uint8))
  with pytest.raises(TypeError, match="torch.uint8"):
    ffpa_attn_amd.unpack_latent_rows_ds(torch.zeros(4, ROW, dtype=torch.int8))


@pytest.mark.parametrize("scales", [(0.37, 3.0e-5, 1234.567, 7.3), (2.0 ** -100 * 1.5, 2.0 ** 100 / 1.5, 1.0, 0.1)])
def test_unpack_is_one_float32_multiply_and_one_rounding_to_bf16_for_every_code(scales):
  """All 256 codes under four scales that are no powers of two, one scale per tile: float64 arithmetic rounded once to float32 and once to bf16."""
  s32 = np.array(scales, dtype=np.float32)
  rows = torch.zeros(2, ROW, dtype=torch.uint8)
  codes = torch.arange(256, dtype=torch.uint8)
  for j in range(4):
    rows[0, 128 * j:128 * (j + 1)], rows[1, 128 * j:128 * (j + 1)] = codes[:128], codes[128:]
  rows[:, 512:528] = torch.from_numpy(np.frombuffer(s32.astype("<f4").tobytes(), dtype=np.uint8).copy())
  rope = torch.randn(2, 64).to(torch.bfloat16)
  rows[:, 528:] = rope.view(torch.uint8)
  got = ffpa_attn_amd.unpack_latent_rows_ds(rows)
  assert torch.equal(got[:, 512:].view(torch.int16), rope.view(torch.int16))
  for j in range(4):
    for code in range(256):
      g = got[code // 128, 128 * j + code % 128]
      v = _e4m3_value(code)
      if math.isnan(v):
        assert torch.isnan(g), (code, j)
        continue
      want = _bf16_rne_bits(np.array([np.float32(v * float(s32[j]))]))[0]  # (float64 product -> float32 -> bf16)
      assert int(g.view(torch.int16)) & 0xFFFF == int(want), (code, j, float(g), v * float(s32[j]))


def test_pack_against_a_plain_python_restatement():
  """Random rows, a row with a zero tile, +-inf, NaN, a tile whose amax sits below the scale floor, a tile without a finite element, a tile of the largest bf16."""
  g = torch.Generator().manual_seed(0)
  kv = (torch.randn(8, 576, generator=g) * torch.tensor([0.01, 1, 30, 1e-3, 1e4, 5, 0.5, 2]).view(8, 1)).to(torch.bfloat16)
  kv[1, 128:256] = 0
  kv[2, 3], kv[2, 200], kv[2, 300] = math.inf, -math.inf, math.nan
  kv[3, 256:384] = 2.0 ** -110
  kv[3, 256] = -(2.0 ** -110)
  kv[4, 384:512] = math.inf
  kv[5, :128] = torch.finfo(torch.bfloat16).max
  kv[6, 520] = math.nan
  kv[7, 5:7] = torch.tensor([0xFFC0 - 0x10000, 0x7FC1], dtype=torch.int16).view(torch.bfloat16)  # (a negative NaN, a NaN with a payload)
  rows = ffpa_attn_amd.pack_latent_rows_ds(kv)
  assert rows[7, 5] == 0xFF and rows[7, 6] == 0x7F
  for r in range(8):
    assert rows[r].numpy().tobytes() == _pack_reference(kv[r]), r
  s = rows[:, 512:528].contiguous().view(torch.float32)
  assert s[1, 1] == 2.0 ** -100 and (rows[1, 128:256] == 0).all()  # the zero tile: the floor, codes +0
  assert rows[2, 3] == 0x7E and rows[2, 200] == 0xFE and rows[2, 300] & 0x7F == 0x7F  # +-inf saturates, NaN stays NaN
  assert s[3, 2] == 2.0 ** -100 and rows[3, 257] == 0x00 and rows[3, 256] == 0x80  # 2^-110 / 2^-100 = 2^-10: the tie goes to +-0
  assert s[4, 3] == 2.0 ** -100 and (rows[4, 384:512] == 0x7E).all()
  assert (rows[5, :128] == 0x7E).all()
  back = ffpa_attn_amd.unpack_latent_rows_ds(rows)
  assert torch.equal(back[:, 512:].view(torch.int16), kv[:, 512:].view(torch.int16))  # rotary bytes round-trip, the NaN included
  fin = [0, 1, 5]
  err = (back[fin, :512].float() - kv[fin, :512].float()).abs().amax() / 1.0
  tile_max = kv[fin, :512].float().abs().view(3, 4, 128).amax(-1, keepdim=True).expand(3, 4, 128).reshape(3, 512)
  assert ((back[fin, :512].float() - kv[fin, :512].float()).abs() <= tile_max * (2.0 ** -4 + 2.0 ** -8)).all(), err  # e4m3's half ulp at the top binade + bf16's


# ----------------------------------------------------------------------------- the Python refusals
def _args(T=3, hq=16, hkv=1, d=576, rows=256, topk=40, paged=False, qdtype=torch.bfloat16, dtype=torch.uint8, last=ROW, device="cpu"):
  q = torch.zeros(T, hq, d, dtype=qdtype, device=device)
  pool = torch.zeros((rows // 16, 16, hkv, last) if paged else (rows, hkv, last), dtype=dtype, device=device)
  idx = torch.zeros(T, topk, dtype=torch.int32, device=device)
  lens = torch.zeros(T, dtype=torch.int32, device=device)
  return q, pool, idx, lens


def _call(q, pool, idx, lens=None, dv=512, **kw):
  kw.setdefault("softmax_scale", SCALE)
  return ffpa_attn_amd.ffpa_attn_with_kvcache_mla_sparse_ds(q, pool, dv, idx, topk_lens=lens, **kw)


@pytest.mark.parametrize("paged", [False, True])
def test_the_refusals_of_the_call_by_type_and_message(paged):
  q, pool, idx, lens = _args(paged=paged)
  for dtype in (torch.float8_e4m3fn, torch.int8, torch.bfloat16):
    with pytest.raises(TypeError, match=f"{CALL} only supports bf16 q over a torch.uint8 kv_cache of 656-byte rows"):
      _call(q, _args(paged=paged, dtype=dtype)[1], idx, lens)
  with pytest.raises(TypeError, match="fp16 q is not served.*torch.float16, torch.uint8"):
    _call(q.half(), pool, idx, lens)
  for last in (576, 640, 672):
    with pytest.raises(ValueError, match=rf"{CALL}: the last dimension of the cache \({last}\) must be the 656 bytes of a row"):
      _call(q, _args(paged=paged, last=last)[1], idx, lens)
  with pytest.raises(NotImplementedError, match=r"\(D, head_dim_v\) = \(576, 448\) is not built"):
    _call(q, pool, idx, lens, dv=448)
  with pytest.raises(NotImplementedError, match=r"\(D, head_dim_v\) = \(512, 512\) is not built"):
    _call(_args(d=512)[0], pool, idx, lens)
  with pytest.raises(TypeError, match=f"{CALL}: softmax_scale is required"):
    ffpa_attn_amd.ffpa_attn_with_kvcache_mla_sparse_ds(q, pool, 512, idx, topk_lens=lens)
  with pytest.raises(NotImplementedError, match=f"{CALL} is inference only: q requires grad"):
    _call(q.clone().requires_grad_(), pool, idx, lens)
  with pytest.raises(NotImplementedError, match=f"{CALL} does not support: kv "):
    _call(q, pool, idx, lens, kv=torch.zeros(3, 1, 576))
  # the sparse call's rules under the new name
  with pytest.raises(NotImplementedError, match=f"{CALL}: per-head index rows"):
    _call(q, pool, idx[:, None].expand(3, 1, 40), lens)
  with pytest.raises(ValueError, match=f"{CALL}: indices must be an int32 tensor"):
    _call(q, pool, idx.long(), lens)
  with pytest.raises(ValueError, match=f"{CALL}: topk_lens must be an int32 tensor"):
    _call(q, pool, idx, lens[:2])
  with pytest.raises(ValueError, match=f"{CALL}: num_splits must be a non-negative int"):
    _call(q, pool, idx, lens, num_splits=-1)
  with pytest.raises(ValueError, match=f"{CALL}: query num_heads"):
    _call(q, _args(paged=paged, hkv=3)[1], idx, lens)
  # T == 0 returns empty tensors and launches nothing
  out, lse = _call(q[:0], pool, idx[:0], lens[:0], return_softmax_lse=True)
  assert out.shape == (0, 16, 512) and lse.shape == (16, 0)


@pytest.mark.parametrize("paged", [False, True])
def test_the_pools_geometry_is_refused_from_sizes_and_strides(paged):
  q, pool, idx, lens = _args(paged=paged, hkv=2)
  wide = torch.zeros(256, 2, ROW + 8, dtype=torch.uint8)[..., :ROW]  # head stride 664: no multiple of 16
  wide = wide.unflatten(0, (16, 16)) if paged else wide
  with pytest.raises(ValueError, match=rf"{CALL}: the slot and head strides of the pool \(1328, 664\) must be multiples of 16 bytes"):
    _call(q, wide, idx, lens)
  mq, _, midx, mlens = _args(device="meta", hq=32)
  ok = torch.empty(256, 2, ROW + 16, dtype=torch.uint8, device="meta")[..., :ROW]  # (a padded slot stride, 672 per head row: served)
  assert _call(mq, ok.unflatten(0, (16, 16)) if paged else ok, midx, mlens).shape == (3, 32, 512)
  overlapping = torch.zeros(256 * 640 + 16, dtype=torch.uint8).as_strided((256, 1, ROW), (640, 640, 1))
  with pytest.raises(ValueError, match="slots at least 656 bytes apart"):
    _call(q[:, :16], overlapping.unflatten(0, (16, 16)) if paged else overlapping, idx, lens)
  if paged:
    uneven = torch.zeros(16, 17, 2, ROW, dtype=torch.uint8)[:, :16]
    with pytest.raises(ValueError, match=f"{CALL}: the pages of kv_cache must be evenly spaced"):
      _call(q, uneven, idx, lens)
  # a pool past 2^31 bytes, from sizes and strides alone (meta tensors own no memory): ValueError before any launch
  rows = ((1 << 31) - ROW) // ROW + 1
  assert rows == 3273603 and (rows - 1) * ROW + ROW <= 1 << 31 < rows * ROW + ROW
  mq, _, midx, mlens = _args(device="meta")
  shape = lambda n: ((n + 15) // 16, 16, 1, ROW) if paged else (n, 1, ROW)
  fits = torch.empty(shape(rows - 15), dtype=torch.uint8, device="meta")
  out = _call(mq, fits, midx, mlens)
  assert out.shape == (3, 16, 512) and out.device.type == "meta"
  big = torch.empty(shape(rows + 16), dtype=torch.uint8, device="meta")
  with pytest.raises(ValueError, match=rf"{CALL}: the pool's rows span \d+ bytes per latent head .* \+ 656\); the sparse call's 32-bit offsets reach at most 2\^31"):
    _call(mq, big, midx, mlens)


def test_the_refusals_of_the_store():
  pool = torch.zeros(64, 1, ROW, dtype=torch.uint8)
  kv = torch.zeros(3, 1, 576, dtype=torch.bfloat16)
  slots = torch.zeros(3, dtype=torch.int32)
  st = ffpa_attn_amd.store_latent_rows_ds
  with pytest.raises(TypeError, match="store_latent_rows_ds only supports bf16 kv over a torch.uint8 kv_cache"):
    st(pool, kv.half(), slots)
  with pytest.raises(TypeError, match="store_latent_rows_ds only supports bf16 kv over a torch.uint8 kv_cache"):
    st(pool.view(torch.int8), kv, slots)
  with pytest.raises(ValueError, match=r"kv must be \[T, Hkv, 576\]"):
    st(pool, kv[..., :512], slots)
  with pytest.raises(ValueError, match=r"kv must be \[T, Hkv, 576\]"):
    st(torch.zeros(64, 2, ROW, dtype=torch.uint8), kv, slots)
  with pytest.raises(ValueError, match=r"slots must be an int32 tensor \[T=3\]"):
    st(pool, kv, slots.long())
  with pytest.raises(ValueError, match="multiples of 16 bytes"):
    st(torch.zeros(64, 1, ROW + 8, dtype=torch.uint8)[..., :ROW], kv, slots)
  assert st(pool.to("meta"), kv.to("meta"), slots.to("meta")) is None  # (the op's fake: nothing to launch)


# ----------------------------------------------------------------------------- the ops' fakes
def test_the_ops_have_fakes_and_compile_on_meta_tensors():
  q = torch.empty(12, 128, 576, dtype=torch.bfloat16, device="meta")
  pool = torch.empty(40, 64, 1, ROW, dtype=torch.uint8, device="meta")
  i32 = lambda *s: torch.empty(s, dtype=torch.int32, device="meta")
  o, lse = torch.ops.ffpa_attn._mla_sparse_ds_fwd_hip(q, pool, 512, i32(12, 300), i32(12), 0.07, 3)
  assert o.shape == (12, 128, 512) and o.dtype == torch.bfloat16 and lse.shape == (128, 12) and lse.dtype == torch.float32
  assert torch.ops.ffpa_attn._mla_ds_store_hip(pool, torch.empty(5, 1, 576, dtype=torch.bfloat16, device="meta"), i32(5)) is None
  schema = str(torch.ops.ffpa_attn._mla_ds_store_hip.default._schema)
  assert "Tensor(a!) kv_cache" in schema  # (the store mutates the pool: a compiler must not reorder the attention call in front of it)

  def f(q, pool, kv, slots, idx, lens):
    ffpa_attn_amd.store_latent_rows_ds(pool, kv, slots)
    out, lse = ffpa_attn_amd.ffpa_attn_with_kvcache_mla_sparse_ds(q, pool, 512, idx, topk_lens=lens, softmax_scale=SCALE, return_softmax_lse=True)
    return out * 2, lse

  args = (q, pool, torch.empty(5, 1, 576, dtype=torch.bfloat16, device="meta"), i32(5), i32(12, 300), i32(12))
  for fn in (f, torch.compile(f, fullgraph=True, backend="eager")):
    out, lse = fn(*args)
    assert out.shape == (12, 128, 512) and out.dtype == torch.bfloat16 and out.device.type == "meta" and lse.shape == (128, 12)


# ----------------------------------------------------------------------------- the C ABI
NEW_SYMBOLS = tuple("ffpa_attn_varlen_mla_sparse_ds_fwd" + s for s in ("", "_plan", "_kernel", "_workspace_bytes")) + ("ffpa_attn_mla_ds_store",)


def test_abi_version_stays_7_and_the_symbols_are_exported_and_declared(lib, tmp_path):
  assert hip.ABI_VERSION == 7 and lib.ffpa_attn_query(0) == 7
  for name in NEW_SYMBOLS:
    assert name in hip.EXPORTS and getattr(lib, name) is not None, name
  header = open(os.path.join(ROOT, "include", "ffpa_attn.h")).read()
  declared = set(re.findall(r"^\s*(?:int|size_t|const char\*)\s+(ffpa_attn_\w+)\s*\(", header, flags=re.M))
  assert set(NEW_SYMBOLS) <= declared and declared == set(hip.EXPORTS)
  src = tmp_path / "decl.c"
  src.write_text('#include <stdio.h>\n#include "ffpa_attn.h"\nint main(void){\nvoid* fns[] = {' + ", ".join(f"(void*){n}" for n in NEW_SYMBOLS) +
                 '};\nprintf("%d %zu %zu\\n", FFPA_ATTN_ABI_VERSION, sizeof(ffpa_mla_ds_store_params), sizeof(fns) / sizeof(fns[0]));\nreturn 0;}\n')
  subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-Wno-pedantic", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "decl.o")], check=True)
  # one new struct, the store's; the attention call takes ffpa_mla_sparse as it is
  assert re.findall(r"typedef struct (\w+)", header).count("ffpa_mla_ds_store_params") == 1 and ctypes.sizeof(hip.FfpaMlaDsStoreParams) == 88
  assert ctypes.sizeof(hip.FfpaMlaSparse) == 64


_KEEP = []


def _buf():
  buf = (ctypes.c_char * 4096)()
  _KEEP.append(buf)
  return (ctypes.addressof(buf) + 15) & ~15


def _c_args(group=16, T=4, topk=64, hkv=1, num_splits=1, flags=0, num_rows=1024, over=None, sover=None, row_bytes=ROW, dtype=torch.bfloat16):
  """The arguments of the sparse exports over a dense pool of ``row_bytes`` per (slot, head) — 656: the new call's; 576: the sparse FP8 call's, 1 byte per element."""
  hq, d, dv = group * hkv, 576, 512
  p, s = hip._mla_sparse_args(dtype, T, hq, hkv, d, dv, topk, num_rows, hkv * row_bytes, row_bytes, (hq * d, d), (hq * dv, dv), SCALE, flags, num_splits)
  base = _buf()
  p.q = p.k = p.o = p.cu_seqlens_q = base
  p.workspace, p.workspace_bytes = base, 0xFFFFFFFFFFFFFFFF
  s.indices = s.topk_lens = base
  for k_, v_ in (over or {}).items():
    setattr(p, k_, (base + v_) if k_ == "k" else v_)
  for k_, v_ in (sover or {}).items():
    if k_ == "kv_stride":
      s.kv_stride[:] = v_
    else:
      setattr(s, k_, v_)
  return (ctypes.byref(p), ctypes.byref(s)), (p, s)


@pytest.mark.parametrize("kw, status, text", [
  # the sparse family's refusals, in its order ...
  (dict(sover=dict(struct_size=56)), 10, b"ffpa_mla_sparse ABI mismatch: size 56 (want 64)"),
  (dict(sover=dict(reserved=1)), 10, b"reserved"),
  (dict(over=dict(abi_version=6)), 10, b"ffpa_varlen_fwd_params ABI mismatch"),
  (dict(over=dict(max_seqlen_q=2)), 4, b"max_seqlen_q=2"),
  (dict(sover=dict(topk=0)), 4, b"topk=0"),
  (dict(sover=dict(indices=None)), 1, b"indices must be non-NULL"),
  (dict(sover=dict(indices_stride=10)), 5, b"indices_stride=10 is smaller than topk=64"),
  (dict(over=dict(dtype=2)), 2, b"dtype"),
  (dict(sover=dict(head_dim_v=448)), 3, b"(576, 448) is not built"),
  # ... then the row format's own, each in front of the next: dtype, strides, base, reach
  (dict(dtype=torch.float16), 2, b"q must be bf16"),
  (dict(dtype=torch.float16, sover=dict(kv_stride=[664, 656])), 2, b"q must be bf16"),
  (dict(sover=dict(kv_stride=[664, 656])), 5, b"kv strides (slot 664, head 656) must be multiples of 16 bytes"),
  (dict(hkv=2, sover=dict(kv_stride=[1328, 664])), 5, b"kv strides (slot 1328, head 664)"),
  (dict(sover=dict(kv_stride=[640, 656])), 5, b"slots at least 656"),
  (dict(sover=dict(kv_stride=[1 << 24, 656])), 5, b"less than 2^24 bytes apart"),
  (dict(sover=dict(kv_stride=[664, 656]), over=dict(k=8)), 5, b"kv strides"),
  (dict(over=dict(k=8)), 6, b"the pool's base must be 16-byte aligned"),
  (dict(over=dict(k=8), num_rows=1 << 23), 6, b"the pool's base must be 16-byte aligned"),
  (dict(num_rows=1 << 23), 4, b"the pool's rows span"),
])
def test_the_statuses_of_the_new_checks_and_their_order(lib, kw, status, text):
  args, keep = _c_args(**kw)
  for fn, extra in ((lib.ffpa_attn_varlen_mla_sparse_ds_fwd, (None,)), (lib.ffpa_attn_varlen_mla_sparse_ds_fwd_plan, ((ctypes.c_int * 5)(),)),
                    (lib.ffpa_attn_varlen_mla_sparse_ds_fwd_kernel, (ctypes.create_string_buffer(200), 200))):
    assert fn(*args, *extra) == status, (fn, lib.ffpa_attn_last_error())
    assert text in lib.ffpa_attn_last_error(), lib.ffpa_attn_last_error()
  assert lib.ffpa_attn_varlen_mla_sparse_ds_fwd_workspace_bytes(*args) == 0


def test_the_reach_is_2_to_the_31_bytes_of_656_byte_rows(lib):
  """(num_rows - 1) x slot stride + 656 <= 2^31: the largest pool within it is accepted, one row more refused — dense rows and rows 1 MiB apart."""
  plan = (ctypes.c_int * 5)()
  exact = ((1 << 31) - ROW) // ROW
  assert exact == 3273602
  args, keep = _c_args(num_rows=exact + 1)
  assert lib.ffpa_attn_varlen_mla_sparse_ds_fwd_plan(*args, plan) == 0, lib.ffpa_attn_last_error()
  args, keep = _c_args(num_rows=exact + 2)
  assert lib.ffpa_attn_varlen_mla_sparse_ds_fwd_plan(*args, plan) == 4 and b"span 2147484224 bytes" in lib.ffpa_attn_last_error()
  stride = 1 << 20
  rows = ((1 << 31) - ROW) // stride + 1
  assert rows == 2048
  args, keep = _c_args(num_rows=rows, sover=dict(kv_stride=[stride, ROW]))
  assert lib.ffpa_attn_varlen_mla_sparse_ds_fwd_plan(*args, plan) == 0, lib.ffpa_attn_last_error()
  args, keep = _c_args(num_rows=rows + 1, sover=dict(kv_stride=[stride, ROW]))
  assert lib.ffpa_attn_varlen_mla_sparse_ds_fwd_plan(*args, plan) == 4 and b"span 2147484304 bytes" in lib.ffpa_attn_last_error()


@pytest.mark.parametrize("group", [16, 72, 128])
@pytest.mark.parametrize("hkv", [1, 2])
def test_the_plan_is_the_sparse_fp8_calls_at_equal_row_counts(lib, group, hkv, monkeypatch):
  monkeypatch.setenv("FFPA_HIP_FAKE_CUS", "256")
  f8 = hip._stamped(hip.FfpaMlaFp8)
  f8.kv_scale = 0.5
  for T, topk in ((1, 2048), (6, 300), (32, 2048), (5, 1)):
    for ns, flags in ((0, 0), (1, 0), (3, hip.FLAG_FORCE_SPLITS), (5, hip.FLAG_FORCE_SPLITS)):
      args, keep = _c_args(group, T, topk, hkv, ns, flags)
      args8, keep8 = _c_args(group, T, topk, hkv, ns, flags, row_bytes=576)
      args8 += (ctypes.byref(f8),)
      got, want = (ctypes.c_int * 5)(), (ctypes.c_int * 5)()
      nd, n8 = ctypes.create_string_buffer(256), ctypes.create_string_buffer(256)
      assert lib.ffpa_attn_varlen_mla_sparse_ds_fwd_plan(*args, got) == 0, lib.ffpa_attn_last_error()
      assert lib.ffpa_attn_varlen_mla_sparse_fp8_fwd_plan(*args8, want) == 0, lib.ffpa_attn_last_error()
      assert list(got) == list(want)
      assert lib.ffpa_attn_varlen_mla_sparse_ds_fwd_workspace_bytes(*args) == lib.ffpa_attn_varlen_mla_sparse_fp8_fwd_workspace_bytes(*args8)
      assert lib.ffpa_attn_varlen_mla_sparse_ds_fwd_kernel(*args, nd, 256) == 0 and lib.ffpa_attn_varlen_mla_sparse_fp8_fwd_kernel(*args8, n8, 256) == 0
      assert nd.value.startswith(b"ffpa_fwd_m16_mla_sparse_ds_kernel<bf16, 576, dv=512") and b"compact" not in nd.value
      assert nd.value == n8.value.replace(b"ffpa_fwd_m16_mla_sparse_fp8_kernel", b"ffpa_fwd_m16_mla_sparse_ds_kernel")


def _store_params(over=None, tokens=4, hkv=1, rows=64):
  p = hip._stamped(hip.FfpaMlaDsStoreParams)
  base = _buf()
  p.kv_new = p.slots = p.kv_cache = base
  p.kv_new_stride[:] = [hkv * 576, 576]
  p.kv_cache_stride[:] = [hkv * ROW, ROW]
  p.tokens, p.heads_kv, p.num_rows, p.head_dim, p.dtype = tokens, hkv, rows, 576, 0
  for k_, v_ in (over or {}).items():
    if k_.endswith("_stride"):
      getattr(p, k_)[:] = v_
    else:
      setattr(p, k_, (base + v_) if k_ in ("kv_new", "kv_cache", "slots") and v_ is not None else v_)
  return p


@pytest.mark.parametrize("over, status, text", [
  (dict(struct_size=80), 10, b"ffpa_mla_ds_store_params ABI mismatch: size 80 (want 88)"),
  (dict(reserved=1), 10, b"reserved"),
  (dict(reserved2=1), 10, b"reserved2"),
  (dict(dtype=1), 2, b"kv_new must be bf16"),
  (dict(head_dim=512), 3, b"head_dim=512"),
  (dict(tokens=-1), 4, b"tokens=-1"),
  (dict(heads_kv=0), 4, b"heads_kv=0"),
  (dict(num_rows=0), 4, b"num_rows=0"),
  (dict(kv_cache=None), 1, b"must be non-NULL"),
  (dict(slots=None), 1, b"must be non-NULL"),
  (dict(kv_cache=8), 6, b"16-byte aligned"),
  (dict(slots=2), 6, b"slots 4-byte aligned"),
  (dict(kv_new_stride=[580, 576]), 5, b"kv_new stride[0]=580"),
  (dict(kv_cache_stride=[664, 656]), 5, b"kv_cache strides (slot 664, head 656)"),
  (dict(kv_cache_stride=[640, 656]), 5, b"slots at least 656 bytes apart"),
])
def test_the_statuses_of_the_store(lib, over, status, text):
  p = _store_params(over)
  assert lib.ffpa_attn_mla_ds_store(ctypes.byref(p), None) == status, lib.ffpa_attn_last_error()
  assert text in lib.ffpa_attn_last_error(), lib.ffpa_attn_last_error()
  assert lib.ffpa_attn_mla_ds_store(None, None) == 1
