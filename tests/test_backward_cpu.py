"""The backward math on a CPU-only box, exact in float64: ``backward._chunked_recompute_backward`` / ``attention_backward(force="recompute")`` and the
packed call's ``varlen._sequence_backward`` against torch autograd through plain ``softmax(scale QK^T + bias, mask) V`` in float64.

Both are plain torch code: in float64 they must agree with autograd to rounding (~1e-13), so any error in the formula — the LSE gradient term, the
tail-aligned causal cut, the GQA reduction, the per-sequence packing, a chunk boundary — shows up orders of magnitude above the 1e-10 tolerance.
The GPU side (the kernel's O / LSE through these functions against float64) is tests/test_backward_f64_gpu.py."""

from types import SimpleNamespace

import pytest
import torch

from ffpa_attn_amd import backward as bw
from ffpa_attn_amd import varlen as vl

F64 = torch.float64
TOL = 1e-10


def _reference(q, k, v, scale, causal, bias=None, keep=None):
  """O, LSE of dense [B, H, N, D] inputs by plain math in their dtype, on their device (autograd-friendly; tests/test_backward_f64_gpu.py uses it too).  Tail-aligned causal mask (keys > row + Nkv - Nq hidden);
  rows with no visible key are O = 0, LSE = -inf with zero gradient — built explicitly, never through a logsumexp of an all -inf row."""
  nq, nkv = q.size(-2), k.size(-2)
  g = q.size(1) // k.size(1)
  kx, vx = k.repeat_interleave(g, 1), v.repeat_interleave(g, 1)
  s = (q @ kx.transpose(-1, -2)) * scale
  if bias is not None:
    s = s + bias
  vis = torch.ones(nq, nkv, dtype=torch.bool, device=q.device)
  if causal:
    vis = torch.arange(nkv, device=q.device).view(1, -1) <= torch.arange(nq, device=q.device).view(-1, 1) + (nkv - nq)
  vis = vis.expand_as(s) if keep is None else vis & keep.expand_as(s)
  live = vis.any(-1, keepdim=True)
  s = s.masked_fill(~vis, float("-inf")).masked_fill(~live, 0.0)
  lse = torch.logsumexp(s, -1, keepdim=True)
  o = (torch.exp(s - lse) @ vx) * live
  return o, lse.masked_fill(~live, float("-inf")).squeeze(-1)


def _finite(lse):
  return torch.where(torch.isfinite(lse), lse, torch.zeros_like(lse))


def _rand(*shape, gen):
  return torch.randn(*shape, dtype=F64, generator=gen)


def _assert_close(name, got, want):
  assert got.dtype == want.dtype and got.shape == want.shape, (name, got.dtype, got.shape, want.shape)
  err = (got - want).abs().max().item() if want.numel() else 0.0
  assert err <= TOL * max(1.0, want.abs().max().item()), f"{name}: max err {err:.3e}"


# ----------------------------------------------------------------------------- dense: attention_backward / _chunked_recompute_backward
DENSE_CASES = {
  # name: (B, Hq, Hkv, Nq, Nkv, causal, bias, bool mask)
  "mha": (2, 3, 3, 37, 37, False, None, False),
  "gqa_causal_cross": (1, 4, 2, 37, 50, True, None, False),  # tail-aligned: Nq < Nkv
  "mqa_causal_self": (2, 4, 1, 40, 40, True, None, False),
  "bias_rows": (2, 4, 2, 33, 45, False, "rows", False),  # [B, 1, Nq, Nkv]: dbias summed over heads
  "bias_heads": (1, 4, 2, 33, 45, True, "heads", False),  # [1, Hq, 1, Nkv]: one row for every query row, under the causal mask
  "bool_mask": (2, 2, 2, 35, 41, False, None, True),  # with two rows that see no key
  "decode_gqa": (2, 8, 2, 1, 29, True, None, False),
}


def _dense_inputs(case, seed=0):
  B, Hq, Hkv, Nq, Nkv, causal, bias_kind, with_mask = DENSE_CASES[case]
  gen = torch.Generator().manual_seed(seed)
  q, k, v = _rand(B, Hq, Nq, 16, gen=gen), _rand(B, Hkv, Nkv, 16, gen=gen), _rand(B, Hkv, Nkv, 16, gen=gen)
  bias = keep = None
  if bias_kind == "rows":
    bias = _rand(B, 1, Nq, Nkv, gen=gen)
  elif bias_kind == "heads":
    bias = _rand(1, Hq, 1, Nkv, gen=gen)
  if with_mask:
    keep = torch.rand(B, 1, Nq, Nkv, generator=gen) < 0.6
    keep[0, 0, 3] = False
    keep[1, 0, Nq - 1] = False
  go, glse = _rand(B, Hq, Nq, 16, gen=gen), _rand(B, Hq, Nq, gen=gen)
  return q, k, v, bias, keep, causal, go, glse


def _dense_reference_grads(q, k, v, bias, keep, causal, scale, go, glse):
  leaves = [t.clone().requires_grad_() for t in (q, k, v)] + ([bias.clone().requires_grad_()] if bias is not None else [])
  o, lse = _reference(*leaves[:3], scale, causal, bias=leaves[3] if bias is not None else None, keep=keep)
  loss = (o * go).sum() + ((_finite(lse) * glse).sum() if glse is not None else 0.0)
  return o.detach(), lse.detach(), torch.autograd.grad(loss, leaves)


@pytest.mark.parametrize("with_lse", [False, True], ids=["o_loss", "o_and_lse_loss"])
@pytest.mark.parametrize("entry", ["attention_backward", "row_chunks"])
@pytest.mark.parametrize("case", list(DENSE_CASES))
def test_recompute_backward_matches_float64_autograd(case, entry, with_lse):
  """dq / dk / dv (/ dbias) of the recompute backward, handed the exact O / LSE, against autograd.  ``row_chunks``: a budget of one byte, so
  every 16 query rows are a chunk of their own (37 rows: chunks of 16, 16, 5) — each chunk's causal offset and bias rows must line up."""
  q, k, v, bias, keep, causal, go, glse = _dense_inputs(case)
  glse = glse if with_lse else None
  scale = 16 ** -0.5
  o, lse, want = _dense_reference_grads(q, k, v, bias, keep, causal, scale, go, glse)
  attn_bias = keep[:, :, :, :] if keep is not None else bias  # (the bool mask as the kernel gets it: the backward builds the additive form)
  if entry == "attention_backward":
    got = bw.attention_backward(go, q, k, v, o, lse, causal=causal, scale=scale, attn_bias=attn_bias, want_bias_grad=bias is not None,
                                force="recompute", dlse=glse)
  else:
    got = bw._chunked_recompute_backward(go, q, k, v, o, lse, causal, scale, bw._additive_bias(attn_bias, F64), bias is not None, budget_bytes=1,
                                         dlse=glse)
  for name, a, b in zip(("dq", "dk", "dv", "dbias"), got, want):
    _assert_close(f"{case} {name}", a, b)
  if bias is None:
    assert got[3] is None
  if keep is not None:  # rows without a visible key: exactly zero
    dead = ~keep.expand(q.size(0), q.size(1), -1, -1).any(-1)
    assert dead.any() and torch.all(got[0][dead] == 0)


def test_lse_gradient_of_rows_without_a_visible_key_is_ignored():
  """A -inf LSE row has P = 0: whatever its dlse (inf from a z-loss on -inf, NaN), it must not turn into NaN in any gradient."""
  q, k, v, _, keep, causal, go, glse = _dense_inputs("bool_mask")
  o, lse, want = _dense_reference_grads(q, k, v, None, keep, causal, 1.0, go, glse)
  dead = ~torch.isfinite(lse)
  assert dead.any()
  for poison in (float("inf"), float("nan"), -1e30):
    got = bw.attention_backward(go, q, k, v, o, lse, causal=False, scale=1.0, attn_bias=keep, force="recompute", dlse=glse.masked_fill(dead, poison))
    for name, a, b in zip(("dq", "dk", "dv"), got, want):
      _assert_close(f"dlse={poison} {name}", a, b)


def test_an_lse_gradient_never_reaches_aten(monkeypatch):
  """The aten op computes rowsum(dO o O) itself and takes no dlse: with one, attention_backward must not try it; forcing aten is an error."""
  q, k, v, _, _, causal, go, glse = _dense_inputs("gqa_causal_cross")
  o, lse, _ = _dense_reference_grads(q, k, v, None, None, causal, 0.25, go, glse)
  monkeypatch.setattr(bw, "_aten_efficient_backward", lambda *a, **kw: pytest.fail("aten tried with an LSE gradient"))
  bw.attention_backward(go, q, k, v, o, lse, causal=causal, scale=0.25, dlse=glse)
  with pytest.raises(NotImplementedError, match="LSE gradient"):
    bw.attention_backward(go, q, k, v, o, lse, causal=causal, scale=0.25, dlse=glse, force="aten")


# ----------------------------------------------------------------------------- packed: _sequence_backward
# (0 queries; 0 keys; Nq > Nk and Nq < Nk under the causal flag; 1-token sequences; a 1-key sequence under 4 queries)
LENS_Q = [0, 5, 7, 1, 9, 3, 4, 2]
LENS_K = [4, 0, 3, 1, 9, 6, 1, 2]
PAD_Q, PAD_K = 3, 2  # packed rows past cu_seqlens[-1]


def _cu(lens):
  return torch.tensor([0, *torch.tensor(lens).cumsum(0).tolist()], dtype=torch.int32)


def _packed_reference(q, k, v, lens_q, lens_k, causal, scale):
  """Per sequence: [T, H, D] packed float64 -> out [T_q, Hq, D], lse [Hq, T_q] (padding rows: 0 / -inf)."""
  out = q.new_zeros(q.shape[:2] + (v.size(-1),))
  lse = q.new_full((q.size(1), q.size(0)), float("-inf"))
  outs, lses = [], []
  qs = ks = 0
  for nq, nk in zip(lens_q, lens_k):
    if nq and nk:
      d = lambda t, a, n: t[a:a + n].transpose(0, 1).unsqueeze(0)  # noqa: E731
      o, l_ = _reference(d(q, qs, nq), d(k, ks, nk), d(v, ks, nk), scale, causal)
      outs.append((qs, nq, o[0].transpose(0, 1), l_[0]))
    qs, ks = qs + nq, ks + nk
  for a, n, o, l_ in outs:  # (assembled without in-place writes into a graph leaf)
    out = torch.cat([out[:a], o, out[a + n:]])
    lse = torch.cat([lse[:, :a], l_, lse[:, a + n:]], dim=1)
  return out, lse


def _packed_inputs(hq, hkv, seed=0):
  gen = torch.Generator().manual_seed(seed)
  tq, tk = sum(LENS_Q) + PAD_Q, sum(LENS_K) + PAD_K
  q, k, v = _rand(tq, hq, 16, gen=gen), _rand(tk, hkv, 16, gen=gen), _rand(tk, hkv, 16, gen=gen)
  return q, k, v, _rand(tq, hq, 16, gen=gen), _rand(hq, tq, gen=gen)


def _packed_reference_grads(q, k, v, causal, scale, go, glse):
  leaves = [t.clone().requires_grad_() for t in (q, k, v)]
  o, lse = _packed_reference(*leaves, LENS_Q, LENS_K, causal, scale)
  nq = sum(LENS_Q)
  loss = (o[:nq] * go[:nq]).sum() + ((_finite(lse[:, :nq]) * glse[:, :nq]).sum() if glse is not None else 0.0)
  return o.detach(), lse.detach(), torch.autograd.grad(loss, leaves)


def _dead_rows(causal):
  """[T_q] bool: query rows of a sequence that see no key (O = 0, LSE = -inf), padding excluded."""
  dead = []
  for nq, nk in zip(LENS_Q, LENS_K):
    cut = nq if nk == 0 else (max(0, nq - nk) if causal else 0)
    dead += [True] * cut + [False] * (nq - cut)
  return torch.tensor(dead + [False] * PAD_Q)


@pytest.mark.parametrize("with_lse", [False, True], ids=["o_loss", "o_and_lse_loss"])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("hq, hkv", [(4, 4), (4, 2), (4, 1)], ids=["mha", "gqa", "mqa"])
def test_sequence_backward_matches_float64_autograd_per_sequence(hq, hkv, causal, with_lse):
  """The packed backward, handed the exact per-sequence O / LSE, against autograd through each sequence alone.  Padding rows of q / k / v and every
  row past cu_seqlens[-1] of O, LSE, dO and dLSE are NaN: they must never be read, and their gradients are exactly 0; so is dq of every row that sees
  no key (its dLSE, here 1e3, is ignored)."""
  q, k, v, go, glse = _packed_inputs(hq, hkv)
  glse = glse if with_lse else None
  scale = 0.3
  o, lse, want = _packed_reference_grads(q, k, v, causal, scale, go, glse)
  nq, nk = sum(LENS_Q), sum(LENS_K)
  dead = _dead_rows(causal)
  assert dead.any() and bool((~dead[:nq]).any())
  nan = float("nan")
  for t in (q, go):
    t[nq:] = nan
  for t in (k, v):
    t[nk:] = nan
  o[nq:], lse[:, nq:] = nan, nan
  if glse is not None:
    glse = glse.clone()
    glse[:, nq:] = nan
    glse[:, dead] = 1e3
  got = vl._sequence_backward(go, q, k, v, o, lse, _cu(LENS_Q), _cu(LENS_K), causal, scale, dlse=glse, force="recompute")
  for name, a, b, n in zip(("dq", "dk", "dv"), got, want, (nq, nk, nk)):
    _assert_close(f"{name}", a[:n], b[:n])
    assert torch.all(a[n:] == 0), f"{name}: padding rows"
  assert torch.all(got[0][dead] == 0), "dq of rows without a visible key"


# ----------------------------------------------------------------------------- the packed autograd Function: which gradients reach the backward
def _float64_packed_op(q, k, v, cu_q, cu_k, max_q, max_k, scale, causal, thr):
  """Stands in for ffpa_attn::_varlen_fwd_hip on CPU float64 (the real op needs the GPU): the exact O / LSE."""
  return _packed_reference(q, k, v, torch.diff(cu_q).tolist(), torch.diff(cu_k).tolist(), bool(causal), scale)


@pytest.fixture
def packed_fn(monkeypatch):
  import ffpa_attn_amd.hip  # noqa: F401 — registers the op namespace before it is patched

  monkeypatch.setattr(torch.ops.ffpa_attn, "_varlen_fwd_hip", _float64_packed_op)
  calls = []
  real = bw.attention_backward
  monkeypatch.setattr(bw, "attention_backward", lambda *a, **kw: calls.append(kw) or real(*a, **kw))
  # (CPU: aten's efficient backward does not exist here — the spy records the attempt and answers with the recompute)
  monkeypatch.setattr(bw, "_aten_efficient_backward", lambda *a: calls.append("aten") or bw._chunked_recompute_backward(*a))

  def run(hq, hkv, causal, loss_fn):
    q, k, v, go, glse = _packed_inputs(hq, hkv, seed=1)
    leaves = [t.clone().requires_grad_() for t in (q, k, v)]
    out, lse = vl._FFPAAttnVarlenFunc.apply(*leaves, _cu(LENS_Q), _cu(LENS_K), max(LENS_Q), max(LENS_K), 0.3, causal, -1.0)
    grads = torch.autograd.grad(loss_fn(out, lse, go, glse), leaves)
    ref = [t.clone().requires_grad_() for t in (q, k, v)]
    o_r, lse_r = _packed_reference(*ref, LENS_Q, LENS_K, causal, 0.3)
    want = torch.autograd.grad(loss_fn(o_r, lse_r, go, glse), ref, allow_unused=True)  # (the LSE alone does not depend on v)
    want = [torch.zeros_like(t) if w is None else w for t, w in zip(ref, want)]
    return grads, want, calls

  return run


LOSSES = {
  "o_only": lambda o, lse, go, glse: (o[:sum(LENS_Q)] * go[:sum(LENS_Q)]).sum(),
  "o_and_lse": lambda o, lse, go, glse: (o[:sum(LENS_Q)] * go[:sum(LENS_Q)]).sum() + (_finite(lse[:, :sum(LENS_Q)]) * glse[:, :sum(LENS_Q)]).sum(),
  "z_loss": lambda o, lse, go, glse: _finite(lse[:, :sum(LENS_Q)]).square().mean(),
}


@pytest.mark.parametrize("loss", list(LOSSES))
@pytest.mark.parametrize("causal", [False, True])
def test_packed_call_lse_is_differentiable_and_an_unused_lse_keeps_the_aten_route(packed_fn, loss, causal):
  """Through the autograd Function: a loss of the LSE alone (z-loss: no gradient reaches O) or of O and the LSE gets its exact gradient and takes the
  recompute route; a loss of O alone hands the backward no dLSE (set_materialize_grads(False)), so every sequence tries aten first, as before."""
  grads, want, calls = packed_fn(4, 2, causal, LOSSES[loss])
  for name, a, b in zip(("dq", "dk", "dv"), grads, want):
    _assert_close(f"{loss} {name}", a, b)
  seqs = sum(1 for nq, nk in zip(LENS_Q, LENS_K) if nq and nk)
  kws = [c for c in calls if c != "aten"]
  assert len(kws) == seqs
  if loss == "o_only":
    assert all(kw["dlse"] is None and kw["force"] is None for kw in kws)
    assert calls.count("aten") == seqs
  else:
    assert all(kw["dlse"] is not None for kw in kws) and "aten" not in calls


def test_packed_backward_with_only_an_lse_gradient_treats_the_output_gradient_as_zero():
  """backward(ctx, None, dlse): what the engine passes when only the LSE was used."""
  q, k, v, _, glse = _packed_inputs(4, 2)
  o, lse = _packed_reference(q, k, v, LENS_Q, LENS_K, True, 0.3)
  ctx = SimpleNamespace(saved_tensors=(q, k, v, o, lse, _cu(LENS_Q), _cu(LENS_K)), causal=True, scale=0.3)
  got = vl._FFPAAttnVarlenFunc.backward(ctx, None, glse)
  want = vl._sequence_backward(torch.zeros_like(o), q, k, v, o, lse, _cu(LENS_Q), _cu(LENS_K), True, 0.3, dlse=glse)
  assert len(got) == 10 and all(g is None for g in got[3:])
  for a, b in zip(got[:3], want):
    assert torch.equal(a, b)


def test_head_dims_past_aten_reach_the_recompute_only(monkeypatch):
  """aten's efficient-attention backward on ROCm returns NaN gradients past D = 512 instead of refusing: such head dims must never reach it."""
  gen = torch.Generator().manual_seed(3)
  D = bw.ATEN_MAX_HEAD_DIM + 64
  q, k, v, go = _rand(1, 2, 9, D, gen=gen), _rand(1, 2, 11, D, gen=gen), _rand(1, 2, 11, D, gen=gen), _rand(1, 2, 9, D, gen=gen)
  o, lse, want = _dense_reference_grads(q, k, v, None, None, True, D ** -0.5, go, None)
  monkeypatch.setattr(bw, "_aten_efficient_backward", lambda *a, **kw: pytest.fail("aten tried past its head dims"))
  got = bw.attention_backward(go, q, k, v, o, lse, causal=True, scale=D ** -0.5)
  for name, a, b in zip(("dq", "dk", "dv"), got, want):
    _assert_close(name, a, b)
  with pytest.raises(NotImplementedError, match="head_dim"):
    bw.attention_backward(go, q, k, v, o, lse, causal=True, scale=D ** -0.5, force="aten")
