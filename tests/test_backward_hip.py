"""The backward kernel's C ABI and routing without a GPU: the three exports exist and are declared, ``ffpa_attn_bwd`` refuses bad calls with a status and a
``last_error`` text before any device work, ``ffpa_attn_bwd_kernel`` names the build a head dim runs in, and ``attention_backward(force="hip")`` names why it
refuses a call outside the kernel's envelope.  The pointers are fake aligned integers: every refusal returns in front of the device check."""

import ctypes
import os
import re

import pytest
import torch

from ffpa_attn_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ffpa_attn_bwd", "ffpa_attn_bwd_workspace_bytes", "ffpa_attn_bwd_kernel")
_KEEP = []


@pytest.fixture(scope="module")
def lib():
  if not hip.library_available():
    from ffpa_attn_amd import build

    build.build()
  return hip.load_library()


def _good(lib, D=576):
  """A call every check accepts: B 2, Hq 4, Hkv 2, (40, 70), bf16, contiguous, every pointer one fake 16-byte aligned address."""
  buf = (ctypes.c_char * 64)()
  _KEEP.append(buf)
  base = (ctypes.addressof(buf) + 15) & ~15
  p = hip._bwd_params(torch.bfloat16, 2, 4, 2, 40, 70, D, True, 0.04)
  for f, t in hip.FfpaBwdParams._fields_:
    if t is ctypes.c_void_p:
      setattr(p, f, base)
  for i, (sq, sk) in enumerate(((4 * 40 * D, 2 * 70 * D), (40 * D, 70 * D), (D, D))):
    for f in ("q", "o", "dout", "dq"):
      getattr(p, f + "_stride")[i] = sq
    for f in ("k", "v", "dk", "dv"):
      getattr(p, f + "_stride")[i] = sk
  p.workspace_bytes = lib.ffpa_attn_bwd_workspace_bytes(ctypes.byref(p))
  return p


def test_the_three_symbols_are_exported_and_declared(lib):
  header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ffpa_attn.h")).read(), flags=re.S)
  for n in NAMES:
    assert n in hip.EXPORTS and getattr(lib, n) is not None and re.search(r"\b" + n + r"\s*\(", header), n
  assert lib.ffpa_attn_query(0) == hip.ABI_VERSION == 7


def test_workspace_is_two_floats_per_padded_row(lib):
  assert _good(lib).workspace_bytes == 2 * 4 * 2 * 4 * 64  # Nq = 40 -> 64 rows


@pytest.mark.parametrize("over, status, word", [
  (None, 1, b"params is NULL"),
  (dict(struct_size=ctypes.sizeof(hip.FfpaBwdParams) - 8), 10, b"ffpa_bwd_params ABI mismatch"),
  (dict(abi_version=6), 10, b"version 6 (want 7)"),
  (dict(head_dim=512), 3, b"head_dim=512"),
  (dict(head_dim=1032), 3, b"head_dim=1032"),
  (dict(head_dim=580), 3, b"multiples of 8"),
  (dict(heads_q=3), 4, b"heads_q a multiple of heads_kv"),
  (dict(workspace_bytes=2 * 4 * 2 * 4 * 64 - 1), 4, b"is less than the 4096 bytes"),
  (dict(dq=None), 1, b"must be non-NULL"),
  (dict(k_stride=4), 5, b"multiple of 8 elements"),
], ids=lambda x: "-".join(f"{k}={v}" for k, v in x.items()) if isinstance(x, dict) else None)
def test_refusals_come_with_a_status_and_a_text_before_device_work(lib, over, status, word):
  p = _good(lib)
  for f, v in (over or {}).items():
    if f.endswith("_stride"):
      getattr(p, f)[2] = v
    else:
      setattr(p, f, v)
  assert lib.ffpa_attn_bwd(None if over is None else ctypes.byref(p), None) == status, lib.ffpa_attn_last_error()
  assert word in lib.ffpa_attn_last_error(), lib.ffpa_attn_last_error()


def test_the_good_call_is_refused_by_the_missing_device_alone(lib):
  if not torch.cuda.is_available():
    assert lib.ffpa_attn_bwd(ctypes.byref(_good(lib)), None) == 9, lib.ffpa_attn_last_error()


@pytest.mark.parametrize("D, build", [(576, 640), (768, 768), (840, 896), (1024, 1024)])
def test_kernel_names_the_build_of_a_head_dim(lib, D, build):
  name = hip.backward_kernel(D, torch.float16)
  assert f"ffpa_bwd_dkdv_kernel<fp16, {build}>" in name and f"ffpa_bwd_dq_kernel<fp16, {build}>" in name and f"d_valid={D}" in name, name


@pytest.mark.parametrize("what, word", [("bias", "attn_mask / bias"), ("dropout", "dropout"), ("D512", "head_dim 512")])
def test_force_hip_names_why_it_refuses(what, word):
  from ffpa_attn_amd.backward import attention_backward

  D = 512 if what == "D512" else 576
  q = torch.empty(1, 2, 16, D, dtype=torch.bfloat16, device="meta")
  kw = dict(causal=False, scale=1.0, force="hip")
  if what == "bias":
    kw["attn_bias"] = torch.zeros(1, 1, 16, 16, dtype=torch.bfloat16, device="meta")
  if what == "dropout":
    kw["dropout"] = (0.1, 0, 0)
  with pytest.raises(NotImplementedError, match=word):
    attention_backward(q, q, q, q, q, torch.empty(1, 2, 16, device="meta"), **kw)
