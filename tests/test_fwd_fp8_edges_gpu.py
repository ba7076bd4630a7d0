"""The FP8 forward where its first tests did not look: every build and both output dtypes bit for bit on the exact cases of tests/fwd_fp8_cases.py (whose
sharpness tests/test_fwd_fp8_cases.py proves without a GPU), the causal and tail seams, the pre-pass on strided, sliced, offset and expanded inputs, the public
call's arguments, degenerate values in the quantiser, a strided output through the C ABI, and scratch past 2^31 bytes."""

import ctypes
import time

import pytest
import torch

import fwd_fp8_cases as fc
import model_values as mv
from ffpa_attn_amd import ffpa_attn_fp8_codes, ffpa_attn_fp8_func, quantize_attn_fp8
from ffpa_attn_amd.interface import FP8_BLOCK_KEYS as K, FP8_BLOCK_ROWS as R
from fwd_fp8_cases import DTYPES, check_against_dequantised
from test_fwd_gpu import hip  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu


def assert_bits(out, c, dtype, name=None):
  """``out`` equals the case's float64 quotient rounded to fp32 and to ``dtype`` in every bit pattern that is a number's; a row without a key is 0."""
  got, want = out.cpu(), fc.expected(c, dtype)
  assert got.dtype == dtype and got.shape == want.shape
  bad = got != want
  assert not bool(bad.any()), (f"{name or c.name} {dtype}: {int(bad.sum())} of {bad.numel()} elements differ, worst by "
                               f"{float((got.double() - c.want)[bad].abs().max()):.3e}, first at {bad.nonzero()[0].tolist()}")
  assert bool((got[~c.live.expand_as(got)] == 0).all())


def run_codes(c, dtype):
  nq, nkv = c.qc.size(2), c.kc.size(2)
  return ffpa_attn_fp8_codes(*fc.scratch(c, "cuda"), seqlen_q=nq, seqlen_kv=nkv, is_causal=c.causal, out_dtype=dtype)


# ----------------------------------------------------------------------------- B1. every build, both output dtypes, exact
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("cid, args", fc.every_build_cases(), ids=[cid for cid, _ in fc.every_build_cases()])
def test_every_build_is_exact(hip, cid, args, dtype):
  c = fc.exact_case(*args)
  assert_bits(run_codes(c, DTYPES[dtype]), c, DTYPES[dtype])
  nq, nkv = args[3], args[4]
  if c.causal and nq > nkv:
    assert not bool(c.live[:, :, : nq - nkv].any())  # (a whole row tile and more without a key: the first workgroup walks no key tile)


# ----------------------------------------------------------------------------- B2. the seams, exact
@pytest.mark.parametrize("gid", list(fc.seam_groups()))
def test_seams_are_exact(hip, gid):
  """Nq and Nkv on, one below and one above the row tile and the key tile, a single row, a single key, ``row0 + off`` on a key-tile boundary: every case's
  carrier sits ON the row's limit, so a limit, an ``edge`` predicate or a tile count that is off by one moves bits (proved on the reference)."""
  for args in fc.seam_groups()[gid]:
    c = fc.exact_case(*args)
    packed = fc.scratch(c, "cuda")
    for dtype in DTYPES.values():
      out = ffpa_attn_fp8_codes(*packed, seqlen_q=args[3], seqlen_kv=args[4], is_causal=c.causal, out_dtype=dtype)
      assert_bits(out, c, dtype)
    if c.causal and args[4] == 1:
      assert int(c.live.sum()) == args[0] * args[1]  # only the last row sees the key


# ----------------------------------------------------------------------------- B3. the pre-pass on what it has not seen
def assert_prepass_is_the_helper(hip, q, k, v, scale, smooth_k):
  want = quantize_attn_fp8(q.cpu(), k.cpu(), v.cpu(), scale, smooth_k)
  got = hip.fp8_quantize(q, k, v, scale * mv.LOG2E, smooth_k)
  for name, g, w in zip(want._fields, got, want[:6]):
    assert g.shape == w.shape and g.dtype == w.dtype, name
    diff = g.cpu() != w
    assert not bool(diff.any()), f"{name}: {int(diff.sum())} of {diff.numel()} differ, first at {diff.flatten().nonzero()[0].item()}"
  return want


@pytest.mark.parametrize("smooth_k", [True, False])
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("D", [384, 448])
def test_prepass_is_the_helper_at_the_other_builds(hip, D, dtype, smooth_k):
  q, k, v = mv.outliers((2, 4, 1, R + 5, 2 * K + 37, D), DTYPES[dtype], seed=D)
  assert_prepass_is_the_helper(hip, q.cuda(), k.cuda(), v.cuda(), 1.3 * D ** -0.5, smooth_k)


def _padded(x, lead, row):
  """``x``'s values in a buffer whose rows are ``row`` elements long, the view starting ``lead`` elements into each row."""
  buf = torch.zeros(*x.shape[:-1], row, dtype=x.dtype, device=x.device)
  view = buf[..., lead : lead + x.size(-1)]
  view.copy_(x)
  return view


def _layouts(q, k, v):
  """name -> (q, k, v views holding the same values, whether ``_rows_last_dim`` hands them on as they are)."""
  B, hq, nq, D = q.shape
  hkv, nkv = k.size(1), k.size(2)
  bnhd = lambda x: x.transpose(1, 2).contiguous().transpose(1, 2)
  proj = torch.cat([x.transpose(1, 2).reshape(B, nq, -1) for x in (q, k, v)], -1)  # [B, N, (Hq + 2 Hkv) D]: Nq = Nkv here
  cut = lambda a, h: proj[..., a * D : (a + h) * D].unflatten(-1, (h, D)).transpose(1, 2)
  one = lambda x: x[:, :1].contiguous().expand(-1, hkv, -1, -1)
  return {
    "[B, N, H, D] transposed": ((bnhd(q), bnhd(k), bnhd(v)), True),
    "slices of one QKV projection": ((cut(0, hq), cut(hq, hkv), cut(hq + hkv, hkv)), True),
    "base + 8, row stride D + 8": ((q, _padded(k, 8, D + 8), _padded(v, 8, D + 8)), True),
    "base + 4 (copied)": ((_padded(q, 4, D + 8), _padded(k, 4, D + 8), _padded(v, 4, D + 8)), False),
    "row stride D + 4 (copied)": ((_padded(q, 0, D + 4), _padded(k, 0, D + 4), _padded(v, 0, D + 4)), False),
    "one KV head expanded": ((q, one(k), one(v)), True),
  }


LAYOUTS = ("[B, N, H, D] transposed", "slices of one QKV projection", "base + 8, row stride D + 8", "base + 4 (copied)", "row stride D + 4 (copied)",
           "one KV head expanded")


@pytest.mark.parametrize("layout", LAYOUTS)
def test_prepass_and_call_on_strided_inputs(hip, layout):
  D, dtype = 320, torch.bfloat16
  q, k, v = (t.cuda() for t in mv.outliers((2, 4, 2, R + 5, R + 5, D), dtype, seed=77))  # (Nq = Nkv: one projection holds all three)
  (qv, kv, vv), as_is = _layouts(q, k, v)[layout]
  assert set(_layouts(q, k, v)) == set(LAYOUTS)
  assert not (qv.is_contiguous() and kv.is_contiguous() and vv.is_contiguous())
  # (the host layer hands a tensor on as it is iff its last dim is contiguous, its other strides are multiples of 8 and its base is 16-byte aligned)
  taken = all(t.stride(-1) == 1 and all(st % 8 == 0 for st in t.stride()[:-1]) and t.data_ptr() % 16 == 0 for t in (qv, kv, vv))
  assert taken == as_is, "the branch of the host layer (as it is / copied) this layout is here for"
  assert_prepass_is_the_helper(hip, qv, kv, vv, D ** -0.5, True)
  for causal in (False, True):
    on_view = ffpa_attn_fp8_func(qv, kv, vv, is_causal=causal, enable_gqa=True)
    on_copy = ffpa_attn_fp8_func(qv.contiguous(), kv.contiguous(), vv.contiguous(), is_causal=causal, enable_gqa=True)
    assert torch.equal(on_view, on_copy) and on_view.is_contiguous()


# ----------------------------------------------------------------------------- B4. the public call's arguments
def _scales(q, k, v, scale, name):
  h = quantize_attn_fp8(q, k, v, scale, True)
  print(f"{name}: log2 q_scale per (batch, head, row tile) {torch.log2(h.q_scale).int().tolist()}  log2 k_scale per (batch, KV head, key tile) "
        f"{torch.log2(h.k_scale).int().tolist()}")
  return h


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("scale", [0.37, None])
@pytest.mark.parametrize("heads", [(2, 2), (4, 2)])
@pytest.mark.parametrize("family", ["outliers", "peaked"])
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("D", [384, 448])
def test_public_call_arguments(hip, D, dtype, family, heads, scale, causal):
  hq, hkv = heads
  q, k, v = mv.FAMILIES[family]((3, hq, hkv, 129, 513, D), DTYPES[dtype], 3000 + D)
  out = ffpa_attn_fp8_func(q.cuda(), k.cuda(), v.cuda(), is_causal=causal, scale=scale, enable_gqa=hq != hkv)
  assert out.dtype == q.dtype and out.shape == q.shape
  name = f"{family} D{D} {dtype} Hq{hq} Hkv{hkv} scale={scale} causal={causal}"
  if not causal:
    _scales(q, k, v, scale, name)
  ratio, _, _ = check_against_dequantised(out, q, k, v, scale, causal, True, name)
  assert ratio <= 1.0


# ----------------------------------------------------------------------------- B5. degenerate values in the quantiser
def _degenerate(what, dtype):
  shape = (1, 4, 2, 70, 200, 256)
  q, k, v = (t.clone() for t in mv.plain(shape, dtype, 41))
  top = float(torch.finfo(dtype).max)
  if what == "all zero":
    q, k, v = torch.zeros_like(q), torch.zeros_like(k), torch.zeros_like(v)
  elif what == "zero q":
    q = torch.zeros_like(q)
  elif what == "constant k":
    k = k[:, :, :1].expand_as(k).contiguous()
  elif what == "zero v channel":
    v[..., 5] = 0
  elif what == "largest v":
    # fp16: +-65504, the format's largest; bf16: 247 x 2^120, the largest bf16 whose code (240, at scale 2^120) times its scale is still a finite bf16 —
    # from 248 x 2^120 on the code rounds to 256 and the DEQUANTISED value is 2^128
    big = 65504.0 if dtype == torch.float16 else 247.0 * 2.0 ** 120
    assert big <= top and torch.tensor(big).to(dtype).item() == big
    v[..., 9] = torch.where(torch.arange(200) % 2 == 0, big, -big).to(dtype)[None, None, :]
  elif what == "top code":
    # exact multiples of 448 x a power of two: amax / 448 has no mantissa bits, the scale is NOT rounded up and the code is the top one, +-448
    q[:, :, :, 3] = 448.0 * 2.0 ** -3
    k[:, :, :, 7] = torch.where(torch.arange(200) % 3 == 0, -448.0 * 2.0 ** -6, 448.0 * 2.0 ** -6).to(dtype)[None, None, :]
    v[..., 11] = torch.where(torch.arange(200) % 2 == 0, 448.0 * 2.0 ** 4, -448.0 * 2.0 ** 4).to(dtype)[None, None, :]
  return q, k, v


DEGENERATE = [("all zero", True), ("zero q", True), ("constant k", True), ("constant k", False), ("zero v channel", True), ("largest v", True), ("top code", False)]


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("what, smooth_k", DEGENERATE, ids=[f"{w}-smooth{int(s)}" for w, s in DEGENERATE])
def test_degenerate_values(hip, what, smooth_k, dtype):
  q, k, v = _degenerate(what, DTYPES[dtype])
  scale = None if what != "top code" else 1.0 / mv.LOG2E  # (q's premultiplier 1: the planted multiples of 448 stay exact)
  h = assert_prepass_is_the_helper(hip, q.cuda(), k.cuda(), v.cuda(), 256 ** -0.5 if scale is None else scale, smooth_k)
  floor = 2.0 ** -22  # pow2_up(1e-4 / 448)
  if what == "all zero":
    assert bool((h.q_scale == floor).all() and (h.k_scale == floor).all() and (h.v_scale == floor).all()) and not bool(h.v_codes.float().any())
  if what == "zero q":
    assert bool((h.q_scale == floor).all())
  if what == "constant k" and smooth_k:
    assert bool((h.k_scale == floor).all()), "k - mean is rounding residue: the floor sets the scale"
  if what == "zero v channel":
    assert bool((h.v_scale[..., 5] == floor).all())
  if what == "largest v":
    assert float(h.v_codes.float()[..., 9].abs().max()) == (256 if dtype == "fp16" else 240) and bool(torch.isfinite(h.v_codes.float() * h.v_scale[:, :, None]).all())
  if what == "top code":
    assert float(h.v_codes.float()[..., 11].abs().min()) == 448 and bool((h.v_scale[..., 11] == 2.0 ** 4).all())
    assert float(h.k_codes.float().abs().max()) == 448 and float(h.q_codes.float().abs().max()) == 448
  for causal in (False, True):
    out = ffpa_attn_fp8_func(q.cuda(), k.cuda(), v.cuda(), is_causal=causal, scale=scale, enable_gqa=True, smooth_k=smooth_k)
    assert bool(torch.isfinite(out).all())
    # (the allowance is never 0 — half an output ulp is floored at |O| = 2^-6 — so the ratio is a number; a NaN ratio fails the comparison below)
    ratio, bound, want = check_against_dequantised(out, q, k, v, scale, causal, smooth_k, f"{what} smooth_k={smooth_k} {dtype} causal={causal}")
    assert bool((bound > 0).all()) and ratio <= 1.0
    # where every code of a V channel is zero the FP8 term of the allowance is exactly 0 and so is the reference: the output must be exactly 0
    dead = (h.v_codes.float() == 0).all(2).repeat_interleave(2, 1)[:, :, None, :].expand_as(out)
    if what in ("all zero", "zero v channel"):
      assert bool(dead.any())
    assert bool((want[dead] == 0).all()) and bool((out.cpu()[dead] == 0).all())


# ----------------------------------------------------------------------------- B6. output strides through the C ABI
def test_strided_output_through_the_c_abi(hip):
  c = fc.exact_case(*fc.O_STRIDE_CASE)
  B, hq, _, nq, nkv, D, causal = fc.O_STRIDE_CASE
  packed = fc.scratch(c, "cuda")
  for dtype in DTYPES.values():
    sentinel = -1024.0
    back = torch.full((B, nq, hq * D + 8), sentinel, dtype=dtype, device="cuda")
    o = back[..., : hq * D].unflatten(-1, (hq, D)).transpose(1, 2)  # [B, H, N, D] over [B, N, H D + 8]
    assert o.shape == (B, hq, nq, D) and o.stride() == (nq * (hq * D + 8), D, hq * D + 8, 1) and o.data_ptr() == back.data_ptr()
    p = hip._fp8_fwd_params(*packed, o, nq, nkv, causal)
    rc = hip._call_on_stream(hip.load_library().ffpa_attn_fp8_fwd, o.device, ctypes.byref(p))
    assert rc == 0, hip.load_library().ffpa_attn_last_error()
    torch.cuda.synchronize()
    assert torch.equal(o, ffpa_attn_fp8_codes(*packed, seqlen_q=nq, seqlen_kv=nkv, is_causal=causal, out_dtype=dtype))
    assert_bits(o, c, dtype)
    assert bool((back[..., hq * D :] == sentinel).all()), "the eight elements behind every row are not the call's"


# ----------------------------------------------------------------------------- B7. scratch past 2^31 bytes
def test_scratch_past_2_31_bytes(hip):
  """K8 and V8T of 264 x 125 tiles of 64 KiB = 2 162 688 000 bytes each, zero codes but for the LAST batch, whose tiles start past byte 2^31: it holds an exact
  case and must come out bit for bit; every other batch is uniform attention over zero V and must be exactly 0."""
  c = fc.exact_case(*fc.WIDE_CASE)
  B, nkv, D = fc.WIDE_B, fc.WIDE_CASE[4], fc.WIDE_CASE[5]
  shapes = hip.fp8_scratch_shapes(B, 1, 1, 1, nkv, D)
  assert shapes["k8"][0] * shapes["k8"][2] * shapes["k8"][3] > 2 ** 31 and (B - 1) * shapes["v8t"][2] * shapes["v8t"][3] > 2 ** 31
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  wide = {n: (torch.ones if n.endswith("scale") else torch.zeros)(s, dtype=torch.float32 if n.endswith("scale") else torch.uint8, device="cuda") for n, s in shapes.items()}
  for n, t in zip(("q8", "q_scale", "k8", "k_scale", "v8t", "v_scale"), fc.scratch(c, "cuda")):
    wide[n][B - 1 :] = t
  out = ffpa_attn_fp8_codes(*(wide[n] for n in ("q8", "q_scale", "k8", "k_scale", "v8t", "v_scale")), seqlen_q=1, seqlen_kv=nkv, is_causal=False, out_dtype=torch.bfloat16)
  torch.cuda.synchronize()
  print(f"scratch past 2^31: {sum(t.numel() * t.element_size() for t in wide.values()) / 2 ** 30:.2f} GiB allocated, filled and attended in {time.perf_counter() - t0:.3f} s")
  assert out.shape == (B, 1, 1, D)
  assert_bits(out[B - 1 :], c, torch.bfloat16)
  assert bool((out[: B - 1] == 0).all())
  del wide, out
  torch.cuda.empty_cache()


# ----------------------------------------------------------------------------- what hip.fp8_forward refuses (behind its is_cuda check)
@pytest.mark.parametrize("what, word", [
  ("q8 shape", r"q8 must be a contiguous torch.uint8 tensor of shape \(1, 2, 1, 16384\)"),
  ("k8 dtype", "k8 must be a contiguous torch.uint8 tensor"),
  ("q_scale dtype", "q_scale must be a contiguous torch.float32 tensor"),
  ("k_scale shape", r"k_scale must be a contiguous torch.float32 tensor of shape \(1, 2, 2\)"),
  ("v8t not contiguous", "v8t must be a contiguous torch.uint8 tensor"),
  ("v_scale device", "v_scale must be a contiguous torch.float32 tensor"),
  ("seqlen_kv", r"k8 must be a contiguous torch.uint8 tensor of shape \(1, 2, 3, 32768\)"),
])
def test_fp8_forward_refuses_wrong_scratch(hip, what, word):
  s = hip.fp8_scratch_shapes(1, 2, 2, 8, 200, 256)
  a = {n: torch.zeros(sh, dtype=torch.float32 if n.endswith("scale") else torch.uint8, device="cuda") for n, sh in s.items()}
  nkv = 200
  if what == "q8 shape":
    a["q8"] = a["q8"][..., :-16].contiguous()
  elif what == "k8 dtype":
    a["k8"] = a["k8"].view(torch.int8)
  elif what == "q_scale dtype":
    a["q_scale"] = a["q_scale"].double()
  elif what == "k_scale shape":
    a["k_scale"] = a["k_scale"][..., :1].contiguous()
  elif what == "v8t not contiguous":
    a["v8t"] = a["v8t"].transpose(1, 2).contiguous().transpose(1, 2)
  elif what == "v_scale device":
    a["v_scale"] = a["v_scale"].cpu()
  elif what == "seqlen_kv":
    nkv = 300
  with pytest.raises(ValueError, match=word):
    hip.fp8_forward(a["q8"], a["q_scale"], a["k8"], a["k_scale"], a["v8t"], a["v_scale"], 8, nkv, False, False)
