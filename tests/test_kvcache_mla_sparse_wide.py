"""``wide_pool=True`` on the three sparse latent calls, without a GPU: the argument checks accept pools past the narrow builds' 2^31 bytes per latent head (meta
tensors: nothing is allocated), ``wide_pool=False`` refuses them as before, and the C ``..._wide_fwd_plan`` / ``_kernel`` — host buffers, only the plan runs —
return the narrow call's plan inside that limit, succeed past it where the narrow call returns FFPA_ERR_BAD_SHAPE, and name the wide kernels."""

import ctypes

import pytest
import torch

import ffpa_attn_amd
from ffpa_attn_amd import hip

SCALE = 192 ** -0.5
# kind -> (the public call, pool dtype, bytes per row, extra keywords, the C calls' stem)
KINDS = {
  "16bit": (ffpa_attn_amd.ffpa_attn_with_kvcache_mla_sparse, torch.bfloat16, 1152, {}, "mla_sparse"),
  "fp8": (ffpa_attn_amd.ffpa_attn_with_kvcache_mla_sparse_fp8, torch.float8_e4m3fn, 576, dict(kv_scale=0.5), "mla_sparse_fp8"),
  "ds": (ffpa_attn_amd.ffpa_attn_with_kvcache_mla_sparse_ds, torch.uint8, 656, {}, "mla_sparse_ds"),
}
_KEEP = []


@pytest.fixture(scope="module")
def lib():
  if not hip.library_available():
    from ffpa_attn_amd import build

    build.build()
  return hip.load_library()


def _rows_past(nbytes, row_bytes):
  return nbytes // row_bytes + 2  # (num_rows - 1) * row bytes + one row > nbytes


@pytest.mark.parametrize("past", [2 ** 31, 2 ** 32])
@pytest.mark.parametrize("kind", KINDS)
def test_the_argument_checks_take_a_pool_past_the_narrow_reach_under_wide_pool_alone(kind, past):
  call, pool_dtype, row_bytes, kw, _ = KINDS[kind]
  q = torch.empty(3, 16, 576, dtype=torch.bfloat16, device="meta")
  idx = torch.empty(3, 40, dtype=torch.int32, device="meta")
  pool = torch.empty(_rows_past(past, row_bytes), 1, row_bytes // pool_dtype.itemsize, dtype=pool_dtype, device="meta")
  out, lse = call(q, pool, 512, idx, softmax_scale=SCALE, return_softmax_lse=True, wide_pool=True, **kw)
  assert out.shape == (3, 16, 512) and out.dtype == torch.bfloat16 and lse.shape == (16, 3)
  with pytest.raises(ValueError, match=r"the pool's rows span \d+ bytes per latent head.*2\^31 = 2147483648.*wide_pool=True"):
    call(q, pool, 512, idx, softmax_scale=SCALE, wide_pool=False, **kw)
  with pytest.raises(ValueError, match=r"2\^31"):
    call(q, pool, 512, idx, softmax_scale=SCALE, **kw)  # (the default is the narrow build)
  with pytest.raises(TypeError, match="wide_pool must be a bool"):
    call(q, pool, 512, idx, softmax_scale=SCALE, wide_pool=None, **kw)


def _plan_args(kind, num_rows, group=16, T=4, topk=2048, num_splits=0):
  """A well-formed sparse call of the kind on host buffers (tests/test_kvcache_mla_sparse.py ``_plan_args``, for the three pools)."""
  row = 656 if kind == "ds" else 576  # the pool's row stride, in its elements
  p, s = hip._mla_sparse_args(torch.bfloat16, T, group, 1, 576, 512, topk, num_rows, row, row, (group * 576, 576), (group * 512, 512), SCALE, 0, num_splits)
  buf = (ctypes.c_char * 4096)()
  base = (ctypes.addressof(buf) + 15) & ~15
  p.q = p.k = p.o = p.cu_seqlens_q = base
  p.workspace, p.workspace_bytes = base, 0xFFFFFFFFFFFFFFFF
  s.indices = s.topk_lens = base
  f8 = hip._stamped(hip.FfpaMlaFp8)
  f8.kv_scale = 0.5
  _KEEP.append((buf, p, s, f8))
  return (ctypes.byref(p), ctypes.byref(s)) + ((ctypes.byref(f8),) if kind == "fp8" else ())


def _plan(lib, stem, args):
  plan, name = (ctypes.c_int * 5)(), ctypes.create_string_buffer(200)
  rc = getattr(lib, f"ffpa_attn_varlen_{stem}_fwd_plan")(*args, plan)
  if rc == 0:
    assert getattr(lib, f"ffpa_attn_varlen_{stem}_fwd_kernel")(*args, name, 200) == 0
  return rc, list(plan), name.value.decode()


@pytest.mark.parametrize("kind", KINDS)
def test_the_c_plan_of_a_wide_call_is_the_narrow_call_s_and_reaches_past_it(lib, kind, monkeypatch):
  monkeypatch.setenv("FFPA_HIP_FAKE_CUS", "256")  # (no device: the plan prices a chip of 256 CUs)
  row_bytes, stem = KINDS[kind][2], KINDS[kind][4]
  for group, num_splits in ((16, 0), (128, 0), (16, 3)):
    args = _plan_args(kind, 32 * 1024, group=group, num_splits=num_splits)
    rc_n, plan_n, name_n = _plan(lib, stem, args)
    rc_w, plan_w, name_w = _plan(lib, stem + "_wide", args)
    assert rc_n == 0 and rc_w == 0, lib.ffpa_attn_last_error()
    assert plan_w == plan_n and name_n.startswith(f"ffpa_fwd_m16_{stem}_kernel<bf16, 576, dv=512")
    assert name_w == name_n.replace(f"{stem}_kernel", f"{stem}_wide_kernel"), (name_n, name_w)
    assert getattr(lib, f"ffpa_attn_varlen_{stem}_wide_fwd_workspace_bytes")(*args) == getattr(lib, f"ffpa_attn_varlen_{stem}_fwd_workspace_bytes")(*args)
  assert plan_n[4] == 3
  for past in (2 ** 31, 2 ** 32):
    args = _plan_args(kind, _rows_past(past, row_bytes))
    assert _plan(lib, stem, args)[0] == 4 and b"2^31 = 2147483648" in lib.ffpa_attn_last_error()  # FFPA_ERR_BAD_SHAPE
    rc_w, plan_w, name_w = _plan(lib, stem + "_wide", args)
    assert rc_w == 0 and plan_w == _plan(lib, stem, _plan_args(kind, 1024))[1] and f"{stem}_wide_kernel" in name_w, lib.ffpa_attn_last_error()
  # every check but the span's is the narrow call's: a row stride at 2^24 elements is refused by both
  args = _plan_args(kind, 1024)
  _KEEP[-1][2].kv_stride[0] = 1 << 24
  assert _plan(lib, stem, args)[0] == _plan(lib, stem + "_wide", args)[0] == 5  # FFPA_ERR_BAD_STRIDE
