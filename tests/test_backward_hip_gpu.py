"""The backward kernel (head dims 513 ... 1024) through ``ffpa_attn_func(..., backward_backend="hip")`` against autograd through plain float64 math, with the
comparator and the constants of test_backward_f64_gpu.py: each of dq / dk / dv within ``C x the SDPA-autograd baseline's error + FLOOR`` in relative Frobenius
norm (C = 2.5 comes from the recompute route's matrix there, not from this kernel).  ``FFPA_BWD_F64_REPORT=<path>`` writes every comparison."""

import math

import pytest
import torch

from test_backward_cpu import _reference
from test_backward_f64_gpu import _compare, _grads, _randn, _report, _sdpa, hip  # noqa: F401  (the fixtures: the library, the report)

pytestmark = pytest.mark.gpu

# (B, Hq, Hkv, Nq, Nkv, causal): the forward takes the kernel at Nq >= 512 or < 8 and Nkv >= 512
SHAPES = {
  "ragged_gqa_batch": (2, 2, 1, 520, 600, False),  # row and key tails, GQA, the batch stride
  "causal_off_grid": (1, 2, 2, 520, 600, True),    # the tail-aligned diagonal off the tile grid
  "rows_without_keys": (1, 4, 1, 640, 512, True),  # the first 128 rows see no key: dq exactly 0
  "short_query": (1, 2, 1, 4, 777, False),
}


def _inputs(shape, D, dtype):
  B, Hq, Hkv, Nq, Nkv, causal = SHAPES[shape]
  seed = D + 7 * Nq
  return (_randn((B, Hq, Nq, D), dtype, seed), _randn((B, Hkv, Nkv, D), dtype, seed + 1), _randn((B, Hkv, Nkv, D), dtype, seed + 2), causal,
          _randn((B, Hq, Nq, D), dtype, seed + 4))


def _library(q, k, v, causal, go, spy=None, **kw):
  """Gradients of ffpa_attn_func; ``spy`` collects the ``force`` of every attention_backward call."""
  from ffpa_attn_amd import backward as bw
  from ffpa_attn_amd import ffpa_attn_func

  real = bw.attention_backward
  if spy is not None:
    bw.attention_backward = lambda *a, **k_: spy.append(k_.get("force")) or real(*a, **k_)
  try:
    leaves = [t.detach().requires_grad_() for t in (q, k, v)]
    out = ffpa_attn_func(*leaves, is_causal=causal, enable_gqa=q.size(1) != k.size(1), **kw)
    return torch.autograd.grad(out, leaves, go)
  finally:
    bw.attention_backward = real


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("D", [576, 584, 768, 1024])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_kernel_gradients_match_float64(hip, shape, D, dtype):
  q, k, v, causal, go = _inputs(shape, D, dtype)
  Nq, Nkv = q.size(2), k.size(2)
  if causal and Nq > Nkv:  # the public call wants Nkv >= Nq under the causal flag: the kernel is reached below it, on the forward kernel's O and LSE
    from ffpa_attn_amd.backward import attention_backward

    o, lse = hip.forward(q, k, v, None, True, D ** -0.5)
    got = attention_backward(go, q, k, v, o, lse, causal=True, scale=D ** -0.5, force="hip")[:3]
    dead = Nq - Nkv
    assert torch.all(got[0][:, :, :dead] == 0), "rows without a visible key get exactly zero"
    q, go, got = q[:, :, dead:], go[:, :, dead:], (got[0][:, :, dead:], got[1], got[2])  # (the references: the rows that see a key)
  else:
    taken = []
    got = _library(q, k, v, causal, go, spy=taken, backward_backend="hip")
    assert taken == ["hip"], taken
  ref = _grads(lambda *t: (_reference(*t, D ** -0.5, causal)[0],), [t.double().requires_grad_() for t in (q, k, v)], [go.double()])
  base = _grads(lambda *t: (_sdpa(*t, causal),), [t.clone().requires_grad_() for t in (q, k, v)], [go])
  _compare(f"hip {shape} D{D}", got, base, ref, record=dict(test="backward_hip", shape=shape, dtype=str(dtype)[6:], D=D, route="hip"))


def test_a_loss_of_o_and_the_lse(hip):
  """dlse reaches the kernel; the baseline of an LSE loss is autograd through float32 math, O and the gradients rounded to the storage dtype."""
  from ffpa_attn_amd.backward import attention_backward

  dtype, D, causal = torch.bfloat16, 768, True
  q, k, v, _, go = _inputs("causal_off_grid", D, dtype)
  glse = _randn(q.shape[:3], torch.float32, 5, math.sqrt(D))
  scale = D ** -0.5
  o, lse = hip.forward(q, k, v, None, causal, scale)
  got = attention_backward(go, q, k, v, o, lse, causal=causal, scale=scale, force="hip", dlse=glse)[:3]

  def math_grads(dt, out_dtype=None):
    leaves = [t.to(dt).requires_grad_() for t in (q, k, v)]
    o_, lse_ = _reference(*leaves, scale, causal)
    o_ = o_ if out_dtype is None else o_.to(out_dtype)
    f = dt if out_dtype is None else torch.float32
    grads = torch.autograd.grad((o_.to(f) * go.to(f)).sum() + (lse_.to(f) * glse.to(f)).sum(), leaves)
    return grads if out_dtype is None else [x.to(out_dtype) for x in grads]

  _compare("hip lse loss D768", got, math_grads(torch.float32, dtype), math_grads(torch.float64),
           record=dict(test="backward_hip_lse", dtype="bfloat16", D=D, route="hip"))


def test_two_calls_return_the_same_bits(hip):
  q, k, v, causal, go = _inputs("ragged_gqa_batch", 1024, torch.bfloat16)
  a, b = (_library(q, k, v, causal, go, backward_backend="hip") for _ in range(2))
  assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_strided_inputs_give_the_contiguous_bits(hip):
  """q / k / v as transposed views of [B, N, H, D] storage are read in place."""
  q, k, v, causal, go = _inputs("causal_off_grid", 584, torch.float16)
  strided = [t.transpose(1, 2).contiguous().transpose(1, 2) for t in (q, k, v)]
  assert not strided[0].is_contiguous()
  a, b = _library(q, k, v, causal, go, backward_backend="hip"), _library(*strided, causal, go, backward_backend="hip")
  assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_outside_the_envelope_the_route_is_todays(hip):
  """A bool mask with backward_backend="hip": the bits of the default backend's route."""
  q, k, v, _, go = _inputs("causal_off_grid", 576, torch.bfloat16)
  mask = torch.rand(q.size(2), k.size(2), device="cuda") > 0.3
  taken = []
  a = _library(q, k, v, False, go, spy=taken, attn_mask=mask, backward_backend="hip")
  b = _library(q, k, v, False, go, attn_mask=mask)
  assert taken == [None] and all(torch.equal(x, y) for x, y in zip(a, b))
