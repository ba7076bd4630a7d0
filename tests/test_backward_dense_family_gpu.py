"""The gradients of ``ffpa_attn_func`` as ONE family against float64 (`pytest -m gpu`, one MI355X): the 48 seeded cases of tests/backward_dense_ref.py — batches
of 2 and 3, GQA, every mask form the public call takes (bool and additive, 16-bit and fp32, 2-D ... 4-D, key padding, ``finfo(float32).min``), ``is_causal``,
dropout next to each of them, bias gradients in every broadcast shape — each through the public call under the backward's three routes (``auto``, aten's op
forced, the recompute forced; ``test_backward_f64_gpu._library_dense`` pins the route and asserts that SDPA never ran).  O and the LSE the backward was handed are
held to float64 with the forward's tolerances (``test_m16_lane_growth_gpu._assert_close``), every gradient with ``test_backward_f64_gpu._compare``, unchanged:
``err_lib <= C err_base + FLOOR`` against the float32 baseline of the reference module.  No tolerance of this file's own.

The reference's dropout mask is ``philox.dropout_keep_mask``; ``test_the_kernel_keeps_exactly_the_elements_philox_py_says`` is what makes that legitimate: the
kernel's own keep decisions, read off O for q = 0 and V = I, equal it as whole tensors at a batch of two, an offset inside a Philox quad and a 62-bit seed.

``FFPA_BWD_F64_REPORT=<path>`` (tests/test_backward_f64_gpu.py) receives this file's comparisons too; the last test prints the worst ratio per route and kind."""

import collections
import math

import numpy as np
import pytest
import torch

import backward_dense_ref as R
from test_backward_f64_gpu import _RECORDS, _compare, _library_dense, _report, hip  # noqa: F401 — (fixtures: the library, and the report written at teardown)
from test_m16_lane_growth_gpu import _assert_close

pytestmark = pytest.mark.gpu

_REF: dict = {}


def _case(seed):
  """A case's tensors on the GPU, its keep mask, float64 reference and float32 baseline: computed once, shared by the routes, never written to."""
  if seed not in _REF:
    _REF.clear()  # (one case's float64 tensors at a time)
    c = R.draw_case(seed)
    t = R.materialize(c, "cuda")
    keep = R.keep_mask(c, t, "cuda")
    _REF[seed] = (c, t, R.reference(c, t, keep=keep), R.baseline(c, t, keep=keep))
  return _REF[seed]


def _through_the_public_call(c, t, seen, m):
  """``_library_dense`` calls ``ffpa_attn_amd.ffpa_attn_func(q, k, v, attn_mask=<its differentiable leaf or None>, is_causal, enable_gqa)``: the wrapper hands
  the call the case's non-differentiable mask and dropout, sets the generator to the case's seed and offset and notes what the call will reserve, and keeps O;
  the spy on ``attention_backward`` keeps the LSE (and the dropout triple) the backward was handed."""
  import ffpa_attn_amd
  from ffpa_attn_amd import backward as bw

  real_call, real_bw = ffpa_attn_amd.ffpa_attn_func, bw.attention_backward

  def call(q, k, v, attn_mask=None, is_causal=False, enable_gqa=False):
    mask = attn_mask if attn_mask is not None else t["mask"]
    assert (attn_mask is not None) == c["bias_grad"]
    p = 0.0
    if t["dropout"] is not None:
      p = t["dropout"][0]
      torch.cuda.manual_seed(c["rng_seed"])
      torch.cuda._set_rng_state_offset(c["rng_offset"])
      seen["rng"] = (p, int(torch.cuda.initial_seed()), int(torch.cuda._get_rng_state_offset()))
    out = real_call(q, k, v, attn_mask=mask, dropout_p=p, is_causal=is_causal, enable_gqa=enable_gqa)
    seen["o"] = out.detach()
    return out

  def backward(*a, **kw):
    seen["lse"], seen["dropout"] = a[5], kw.get("dropout")
    return real_bw(*a, **kw)

  m.setattr(ffpa_attn_amd, "ffpa_attn_func", call)
  m.setattr(bw, "attention_backward", backward)


@pytest.mark.parametrize("seed", R.SWEEP_SEEDS)
def test_dense_family_gradients_match_float64(hip, seed, monkeypatch):
  c, t, ref, base = _case(seed)
  dtype = R.DTYPES[c["dtype"]]
  bias = t["mask"] if c["bias_grad"] else None
  names = ("dq", "dk", "dv", "dbias")
  record = dict(test="dense_family", seed=seed, kind=c["kind"], dtype=c["dtype"], D=c["D"], B=c["B"], heads="%d/%d" % c["heads"], Nq=c["Nq"], Nkv=c["Nkv"],
                dropout_p=c["dropout_p"], bias_grad=c["bias_grad"])
  failures, auto_route = [], None
  for force in (None, "aten", "recompute"):
    tag = f"family seed {seed} {c['kind']} {c['dtype']} D{c['D']} {force or 'auto'}"
    seen = {}
    with monkeypatch.context() as m:
      _through_the_public_call(c, t, seen, m)
      try:
        got, route = _library_dense(t["q"], t["k"], t["v"], bias, c["causal"], t["go"], force, monkeypatch)
      except (RuntimeError, NotImplementedError) as e:
        # aten's op (or the rule that keeps a case away from it) refuses: then auto must have taken the recompute, and the forced recompute covers the case
        assert force == "aten" and auto_route == "recompute", (tag, auto_route, e)
        _RECORDS.append(dict(record, auto_route=auto_route, route="aten", refused=str(e).splitlines()[0][:160]))
        continue
    if force is None:
      auto_route = route
      record["auto_route"] = route
    if t["dropout"] is not None:
      # the call reserved what the reference drew its mask from, and only the recompute rebuilds the kernel's mask
      assert seen["rng"] == t["dropout"] and tuple(seen["dropout"]) == t["dropout"] and route == "recompute", (tag, seen["rng"], seen["dropout"], route)
    else:
      assert force is None or route == force, (tag, route)
    try:
      _assert_close(seen["o"], seen["lse"], ref["o"], ref["lse"], dtype, tag)
      if bias is not None:
        assert got[3].shape == bias.shape and got[3].dtype == bias.dtype, (tag, got[3].shape, got[3].dtype)
      _compare(tag, got, base["grads"], ref["grads"], names, dict(record, route=force or "auto", took=route))
    except AssertionError as e:
      failures.append(str(e).splitlines()[0])
      # (the comparator stops at the first gradient past the bound: put the others of this route on record too)
      for n, g, b, r in zip(names, got, base["grads"], ref["grads"]):
        try:
          _compare(tag + " (after a failure)", (g,), (b,), (r,), (n,), dict(record, route=force or "auto", took=route, after_failure=True))
        except AssertionError:
          pass
  assert not failures, "\n".join(failures)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_rows_padded_on_every_key_with_finfo_min_come_out_as_the_forward_computed_them(hip, dtype, monkeypatch):
  """An fp32 padding mask holding finfo(float32).min with rows that carry it on EVERY key (``test_backward_dense_family.padded_rows_case``), D 512 and a row
  count aten's op serves.  Converted to the queries' dtype the value is -inf, and the row NaN; the forward computes such a row as uniform attention (the
  documented contract) and hands the backward an LSE of finfo(float32).min.  Every gradient, and dq of those rows alone, against float64 on every route."""
  from test_backward_dense_family import padded_rows_case

  c, t = padded_rows_case(dtype, 520, 600, 512, torch.finfo(torch.float32).min, "cuda")
  ref, base = R.reference(c, t), R.baseline(c, t)
  rows = lambda g: [g[0][1, :, :3]]  # noqa: E731
  assert ref["grads"][0][1, :, :3].norm().item() > 0.0
  auto_route = None
  for force in (None, "aten", "recompute"):
    tag = f"padded rows {dtype} {force or 'auto'}"
    seen = {}
    with monkeypatch.context() as m:
      _through_the_public_call(c, t, seen, m)
      try:
        got, route = _library_dense(t["q"], t["k"], t["v"], None, False, t["go"], force, monkeypatch)
      except (RuntimeError, NotImplementedError) as e:
        assert force == "aten" and auto_route == "recompute", (tag, auto_route, e)
        continue
    auto_route = auto_route or route
    # (the kernel writes the LSE of a saturated row as -2^100 / l — finite, below -2^60: csrc/ffpa_common.h ``row_lse`` —, float64 holds finfo.min there:
    # asserted finite and that far down, then left out of the comparison, as tests/model_values.py ``check_case`` does)
    lse = seen["lse"].clone()
    assert bool(torch.isfinite(lse[1, :, :3]).all()) and bool((lse[1, :, :3] < -2.0 ** 60).all()) and bool((lse[0].abs() < 100).all())
    lse[1, :, :3] = ref["lse"][1, :, :3].float()
    _assert_close(seen["o"], lse, ref["o"], ref["lse"], R.DTYPES[dtype], tag)
    record = dict(test="dense_family", seed=-1, kind="fp32_padded_rows", dtype=dtype, D=512, route=force or "auto", took=route)
    _compare(tag, got, base["grads"], ref["grads"], record=record)
    _compare(tag + ": their dq", rows(got), rows(base["grads"]), rows(ref["grads"]), names=("dq",), record=dict(record, rows="padded"))


# ----------------------------------------------------------------------------- the kernel's keep mask, exactly
KEEP_SHAPES = [(512, 512), (1024, 1024), (777, 1024)]  # (Nkv, D): the D <= 512 build; the split-D build; a ragged last KV tile, Nkv no multiple of 4
KEEP_P = [0.1, 0.5, float(np.nextafter(np.float32(0.5), np.float32(1.0))), 2.0 ** -24]
KEEP_SEED = (1 << 61) + 0x0123_4567_89AB_CDEF  # 62 bits
KEEP_OFFSET = 4 * ((1 << 33) + 5) + 1          # = 1 mod 4, past 2^32: every group of four elements straddles two Philox blocks


@pytest.mark.parametrize("p", KEEP_P, ids=["p0.1", "p0.5", "p0.5+ulp", "p2^-24"])
@pytest.mark.parametrize("nkv, D", KEEP_SHAPES, ids=[f"Nkv{n}-D{d}" for n, d in KEEP_SHAPES])
def test_the_kernel_keeps_exactly_the_elements_philox_py_says(hip, nkv, D, p):
  """q = 0 makes P uniform and positive, V = I puts P[b, h, r, j] o keep / (1 - p) into O[b, h, r, j]: O != 0 exactly where the kernel kept element
  (b, h, r, j).  The whole boolean tensor against ``dropout_keep_mask`` at B 2, heads 4 / 2, 130 rows (a full 128-row tile and a ragged one).  No backward runs:
  this is the statement a change to the kernel's dropout is checked against."""
  from ffpa_attn_amd.philox import dropout_keep_mask

  assert KEEP_SEED.bit_length() == 62 and KEEP_OFFSET % 4 == 1
  B, hq, hkv, nq = 2, 4, 2, 130
  dtype = torch.bfloat16 if D == 512 or nkv == 777 else torch.float16
  g = torch.Generator(device="cuda").manual_seed(nkv + D)
  q = torch.zeros(B, hq, nq, D, dtype=dtype, device="cuda")
  k = torch.randn(B, hkv, nkv, D, dtype=torch.float32, device="cuda", generator=g).to(dtype)
  v = torch.eye(nkv, D, dtype=dtype, device="cuda").expand(B, hkv, nkv, D).contiguous()
  o, _ = hip.forward(q, k, v, None, False, D ** -0.5, dropout_p=p, philox_seed=KEEP_SEED, philox_offset=KEEP_OFFSET)
  assert o.shape == (B, hq, nq, D) and torch.all(o[..., nkv:] == 0) and bool(torch.isfinite(o).all())
  kept = o[..., :nkv] != 0
  want = dropout_keep_mask(KEEP_SEED, KEEP_OFFSET, R.element_index(dict(B=B, heads=(hq, hkv), Nq=nq, Nkv=nkv), "cuda"), p)
  wrong = int((kept != want).sum())
  assert torch.equal(kept, want), f"{wrong} of {want.numel()} keep decisions differ"
  # ... and not all kept: the kept share within four binomial standard deviations of 1 - p
  n = want.numel()
  share = kept.double().mean().item()
  assert abs(share - (1.0 - p)) <= 4.0 * math.sqrt(p * (1.0 - p) / n), (share, p, n)
  assert torch.all(o[..., :nkv][kept] > 0)


# ----------------------------------------------------------------------------- the report
def test_zz_report_worst_ratio_per_route_and_mask_kind():
  """Not a check of the kernels: prints, per route and per mask kind, the worst err_lib / err_base this run saw (``refused``: aten's op did not serve it)."""
  worst, refused = collections.defaultdict(float), collections.Counter()
  for r in _RECORDS:
    if r.get("test") == "dense_family":
      if "refused" in r:
        refused[r["kind"]] += 1
      else:
        key = (r["route"] + ("" if r["route"] == r["took"] else " -> " + r["took"]), r["kind"])
        worst[key] = max(worst[key], r["ratio"])
  for (route, kind), ratio in sorted(worst.items()):
    print(f"[ratio] {route:22s} {kind:16s}: {ratio:.3f}")
  for kind, n in sorted(refused.items()):
    print(f"[aten refused] {kind:16s}: {n} cases")
  assert all(math.isfinite(x) for x in worst.values())
