"""The dense-gradient sweep's generator, float64 reference and comparator (tests/backward_dense_ref.py, ``test_backward_f64_gpu._compare``), judged without a GPU
on small copies of the sweep's own cases (``backward_dense_ref.shrink``): the coverage of the committed seeds; that no case is vacuous (its mask and its
dropout each move the float64 dq by more than the comparator allows); that the comparator, fed ``backward._chunked_recompute_backward`` on the exact O / LSE
in float64 with ONE thing wrong at a time, rejects it — the fp32 bias rounded to the queries' dtype before the recompute (what
``backward._aten_efficient_backward`` did before an fp32 bias was kept away from it), the dropout index without its batch term, ``keep`` not rescaled in dV,
dbias summed over the wrong broadcast dimension, a key-padding length off by one —; and ``philox.dropout_keep_mask`` against the C oracle's Philox at elements of
a batch of two (tests/test_dropout_cpu.py checks seven elements of one (batch, head) slice at a 61-bit seed: no batch or head term)."""

import collections
import random

import numpy as np
import pytest
import torch

import backward_dense_ref as R
from ffpa_attn_amd import backward as bw
from ffpa_attn_amd.philox import dropout_keep_mask
from oracle import ffpa_oracle as fo
from test_backward_f64_gpu import C, _compare, _rel  # (the comparator and its bound: nothing of that file runs here)

CASES = [R.draw_case(s) for s in R.SWEEP_SEEDS]
F64 = torch.float64
_MADE: dict = {}


def _made(c):
  """A small copy of a case, its CPU tensors, float64 reference and float32 baseline: made once and shared (nothing writes to them)."""
  key = tuple(sorted((k, str(v)) for k, v in c.items()))
  if key not in _MADE:
    t = R.materialize(c)
    _MADE[key] = (t, R.reference(c, t), R.baseline(c, t))
  return _MADE[key]


# ----------------------------------------------------------------------------- the generator
def test_the_seed_list_covers_every_axis():
  assert R.SWEEP_SEEDS == tuple(range(48)) and len(R.KINDS) == 12
  for kind in R.KINDS:
    mine = [c for c in CASES if c["kind"] == kind]
    assert {(c["dtype"], c["d_class"]) for c in mine} == {(d, k) for d in ("bf16", "fp16") for k in (0, 1)}, kind
  assert all(c["D"] in R.D_CLASSES[c["d_class"]] for c in CASES) and {c["D"] for c in CASES} == {320, 456, 512, 576, 768, 1024}
  assert {c["B"] for c in CASES} == {2, 3} and {c["heads"] for c in CASES} == set(R.HEADS)
  # every additive bias shape (16-bit and fp32: rows, full, heads) once with a bias gradient, in both head-dim classes between them; a 3-D one too
  grad = [c for c in CASES if c["bias_grad"]]
  assert collections.Counter(c["kind"] for c in grad) == collections.Counter(R.ADDITIVE + ("lowdim",))
  assert {c["d_class"] for c in grad if c["kind"].startswith("fp32")} == {0, 1}
  forms = {(R.mask_form(c)[0], len(R.mask_form(c)[1])) for c in CASES if c["kind"] == "lowdim"}
  assert {n for _, n in forms} == {2, 3} and {v for v, _ in forms} == {"add16", "fp32", "bool"}
  assert sum(c["alibi"] for c in CASES) == 1 and all(c["Nq"] == 1 and c["kind"] == "fp32_heads" for c in CASES if c["alibi"])
  # shapes: what the kernel serves (functional.py: Nkv >= 512 and Nq >= 512 or Nq <= 7); both decode lengths; key counts no multiple of 8; the edges
  for c in CASES:
    assert c["Nkv"] >= 512 and (512 <= c["Nq"] <= 640 or c["Nq"] in (1, 5)) and (c["Nkv"] <= 777 or (c["decode"] and c["Nkv"] == 4096)), c
    assert not c["causal"] or c["Nkv"] >= c["Nq"]
    assert 3 * 8 * 640 * 777 * 8 >= c["B"] * c["heads"][0] * c["Nq"] * c["Nkv"] * 8  # the largest float64 score tensor: 95 MB
  decode = [c for c in CASES if c["decode"]]
  assert len(decode) == 12 and {c["Nq"] for c in decode} == {1, 5} and {c["Nkv"] == 4096 for c in decode} == {False, True}
  assert {c["Nq"] for c in decode if c["Nkv"] == 4096} == {1, 5}
  assert sum(c["Nkv"] % 8 != 0 for c in CASES) >= 16 and sum(c["Nkv"] % 2 != 0 for c in CASES) >= 8
  assert {512, 640} <= {c["Nq"] for c in CASES} and {512, 777} <= {c["Nkv"] for c in CASES}
  # every mask kind, and every fp32 bias shape, in a case aten's backward can serve (D <= 512, rows a multiple of 8, no dropout) — and rows that are no
  # multiple of 8 next to them
  may = [c for c in CASES if c["aten_may_serve"]]
  assert {c["kind"] for c in may} == set(R.KINDS) and all(c["Nq"] % 8 == 0 and c["D"] <= 512 and c["dropout_p"] == 0.0 for c in may)
  assert {c["dtype"] for c in may if R.mask_form(c)[0] == "fp32"} == {"bf16", "fp16"} and any(c["bias_grad"] for c in may if R.mask_form(c)[0] == "fp32")
  assert sum(c["Nq"] % 8 != 0 for c in CASES if not c["decode"]) >= 8
  # key padding: left and right, every batch keeps a key
  for c in CASES:
    if "keypad" in c["kind"]:
      assert {side for side, _ in c["pad"]} == {"left", "right"} and all(1 <= e - a < c["Nkv"] for a, e in R.kept_keys(c)), c
  # dropout: one case in three, both probabilities, with is_causal, a bool mask and an fp32 bias at least twice each, nonzero generator offsets
  drop = [c for c in CASES if c["dropout_p"] > 0.0]
  assert len(drop) == 16 and {c["dropout_p"] for c in drop} == {0.1, 0.5}
  assert sum(c["causal"] for c in drop) >= 2 and sum(R.mask_form(c)[0] == "bool" for c in drop) >= 2 and sum(R.mask_form(c)[0] == "fp32" for c in drop) >= 2
  assert all(c["rng_offset"] % 4 == 0 for c in drop) and sum(c["rng_offset"] > 0 for c in drop) >= 8 and any(c["rng_offset"] >= 1 << 32 for c in drop)
  assert any(c["rng_seed"] >= 1 << 61 for c in drop) and {c["d_class"] for c in drop} == {0, 1} and {c["dtype"] for c in drop} == {"bf16", "fp16"}
  assert any(c["B"] == 3 for c in drop) and any(c["heads"][0] != c["heads"][1] for c in drop)


def test_the_small_copies_keep_what_the_cases_are_about():
  for c in CASES:
    s = R.shrink(c)
    assert all(s[k] == c[k] for k in ("kind", "dtype", "B", "heads", "causal", "dropout_p", "bias_grad", "pad", "rng_seed", "rng_offset"))
    assert s["Nkv"] > s["Nq"] and (s["Nq"] == c["Nq"] or c["Nq"] >= 512)
    t = R.materialize(s)
    values, shape = R.mask_form(s)
    assert (t["mask"] is None) == (values is None) and (t["mask"] is None or tuple(t["mask"].shape) == shape)
    if values is not None:
      assert t["mask"].dtype == {"bool": torch.bool, "add16": R.DTYPES[c["dtype"]], "fp32": torch.float32, "fp32_min": torch.float32}[values]
    if values == "fp32_min":  # the value that a conversion to 16 bits turns into -inf, in both dtypes
      assert t["mask"].min().item() == torch.finfo(torch.float32).min and torch.isinf(t["mask"].to(R.DTYPES[c["dtype"]]).min())
    if values == "fp32" and not c["alibi"]:  # an fp32 bias that a conversion to the queries' dtype changes
      assert not torch.equal(t["mask"].to(R.DTYPES[c["dtype"]]).float(), t["mask"])


# ----------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("seed", R.SWEEP_SEEDS)
def test_recompute_backward_in_float64_is_the_reference(seed):
  """``attention_backward(force="recompute")`` handed the reference's O / LSE and float64 inputs agrees with the reference's autograd to rounding, for every
  case of the sweep (batch term of the dropout index, GQA, every mask form and bias-gradient shape): the two were written apart."""
  c = R.shrink(CASES[seed])
  t, ref, _ = _made(c)
  bias = R.mask4(c, t["mask"])
  if bias is not None and bias.dtype != torch.bool:
    bias = bias.double()
  got = bw.attention_backward(t["go"].double(), t["q"].double(), t["k"].double(), t["v"].double(), ref["o"], ref["lse"], causal=c["causal"], scale=c["D"] ** -0.5,
                              attn_bias=bias, want_bias_grad=c["bias_grad"], force="recompute", dropout=t["dropout"])
  for name, a, b in zip(("dq", "dk", "dv", "dbias"), got, ref["grads"]):
    assert (a.reshape(b.shape) - b).abs().max().item() <= 1e-10 * max(1.0, b.abs().max().item()), (seed, name)
  assert (got[3] is not None) == c["bias_grad"]


@pytest.mark.parametrize("seed", [s for s in R.SWEEP_SEEDS if CASES[s]["kind"] != "none" or CASES[s]["dropout_p"] > 0.0])
def test_no_case_is_vacuous(seed):
  """The mask of a case, and its dropout, each move the float64 dq by more than C x the baseline's error against float64: a backward that dropped the
  feature could not pass the comparator."""
  c = R.shrink(CASES[seed])
  _, ref, base = _made(c)
  allowed = C * _rel(base["grads"][0], ref["grads"][0])
  offs = ([("mask", R.features_off(c, dropout=False))] if c["kind"] != "none" else []) + ([("dropout", R.features_off(c, mask=False))] if c["dropout_p"] > 0.0 else [])
  for name, off in offs:
    t_off = R.materialize(off)
    moved = _rel(R.reference(off, t_off)["grads"][0], ref["grads"][0])
    assert moved > allowed, (seed, name, moved, allowed)


# ----------------------------------------------------------------------------- the comparator bites
def _recompute(c, t, ref, **kw):
  """``_chunked_recompute_backward`` in float64 on the exact O / LSE; ``kw`` replaces arguments (the wrong ones)."""
  bias = kw.pop("bias", R.mask4(c, t["mask"]))
  bias = bw._additive_bias(bias, F64)
  bias = bias.double() if bias is not None else None
  q, k, v, go = (kw.pop(n, t[n]).double() for n in ("q", "k", "v", "go"))
  got = bw._chunked_recompute_backward(go, q, k, v, kw.pop("o", ref["o"]), kw.pop("lse", ref["lse"]), c["causal"], c["D"] ** -0.5, bias,
                                       kw.pop("want_bias_grad", c["bias_grad"]), dropout=kw.pop("dropout", t["dropout"]))
  assert not kw
  return [x for x in got if x is not None]


def _shaped(grads, ref):
  return [g.reshape(r.shape) for g, r in zip(grads, ref["grads"])]


def _rejected(name, c, t, ref, base, wrong):
  _compare(f"correct ({name})", _shaped(_recompute(c, t, ref), ref), base["grads"], ref["grads"])
  with pytest.raises(AssertionError, match="err_lib"):
    _compare(name, _shaped(wrong, ref), base["grads"], ref["grads"])


def _first(pred):
  return next(c for c in CASES if pred(c))


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("kind", ["fp32_rows", "fp32_full", "fp32_heads"])
def test_comparator_rejects_an_fp32_bias_rounded_to_the_queries_dtype(kind, dtype):
  """The suspected fault: the LSE belongs to the fp32 bias, P is recomputed from the bias rounded to 16 bits.  At the sweep's own values (~ N(0, 2)), on the
  cases that draw them: this is how it is known that the GPU sweep sees it."""
  c = R.shrink(_first(lambda c: c["kind"] == kind and c["dtype"] == dtype and not c["alibi"] and c["dropout_p"] == 0.0 and not c["decode"]))
  t, ref, base = _made(c)
  rounded = t["mask"].to(R.DTYPES[dtype])
  assert not torch.equal(rounded.float(), t["mask"])
  _rejected(f"bias rounded to {dtype} ({kind})", c, t, ref, base, _recompute(c, t, ref, bias=R.mask4(c, rounded)))


@pytest.mark.parametrize("seed", [s for s in R.SWEEP_SEEDS if CASES[s]["dropout_p"] > 0.0][::3])
def test_comparator_rejects_a_dropout_index_without_its_batch_term(seed):
  """Every batch element recomputed alone (B = 1: the index ``((0 Hq + h) Nq + r) Nkv + j``) with the call's seed and offset: batch 0's mask everywhere."""
  c = R.shrink(CASES[seed])
  t, ref, base = _made(c)
  assert c["B"] > 1
  parts = []
  for b in range(c["B"]):
    one = dict(c, B=1, pad=c["pad"][b:b + 1])
    sl = lambda x: x if x is None or x.dim() != 4 or x.size(0) == 1 else x[b:b + 1]  # noqa: E731
    tb = {n: sl(x) if torch.is_tensor(x) else x for n, x in t.items()}
    tb["mask"] = sl(R.mask4(c, t["mask"]))
    parts.append(_recompute(one, tb, {"o": ref["o"][b:b + 1], "lse": ref["lse"][b:b + 1]}))
  wrong = [torch.cat([p[i] for p in parts]) for i in range(3)]
  if c["bias_grad"]:
    full = [p[3] for p in parts]
    wrong.append(torch.cat(full) if R.mask4(c, t["mask"]).size(0) > 1 else sum(full))
  _rejected("no batch term", c, t, ref, base, wrong)


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_comparator_rejects_a_dv_whose_keep_mask_is_not_rescaled(p):
  c = R.shrink(_first(lambda c: c["dropout_p"] == p))
  t, ref, base = _made(c)
  good = _recompute(c, t, ref)
  _rejected("keep not rescaled in dV", c, t, ref, base, [good[0], good[1], good[2] * (1.0 - p)] + good[3:])


@pytest.mark.parametrize("kind", ["add16_heads", "fp32_heads"])
def test_comparator_rejects_a_dbias_summed_over_the_wrong_dimension(kind):
  """A ``[1, Hq, 1, Nkv]`` bias: dbias is dS summed over the batch and the ROWS; summed over the batch and the HEADS it has — at Nq = Hq — the same shape."""
  c = _first(lambda c: c["kind"] == kind and c["bias_grad"])
  c = R.shrink(c, Nq=c["heads"][0])
  t, ref, base = _made(c)
  full = R.mask4(c, t["mask"]).expand(c["B"], c["heads"][0], c["Nq"], c["Nkv"]).contiguous()
  ds = _recompute(c, t, ref, bias=full)[3]
  assert torch.allclose(ds.sum((0, 2)).double(), ref["grads"][3].double().reshape(c["heads"][0], c["Nkv"]), rtol=1e-9, atol=1e-12)
  good = _recompute(c, t, ref)
  _rejected("dbias over the wrong dimension", c, t, ref, base, good[:3] + [ds.sum((0, 1)).to(good[3].dtype)])


@pytest.mark.parametrize("kind", ["bool_keypad", "fp32_keypad_min"])
def test_comparator_rejects_a_key_padding_length_off_by_one(kind):
  c = R.shrink(_first(lambda c: c["kind"] == kind and c["dropout_p"] == 0.0))
  t, ref, base = _made(c)
  longer = R.materialize(dict(c, pad_delta=1))["mask"]
  assert int((longer != t["mask"]).sum()) == c["B"]
  _rejected("key padding off by one", c, t, ref, base, _recompute(c, t, ref, bias=longer))


def test_the_rounded_bias_is_a_subtle_fault():
  """The rounded fp32 bias is caught by a margin, not by miles: its worst gradient lies between C and 4 C baseline errors, so a comparator four times looser
  would let it pass (and the rejection test above would fail)."""
  for dtype in ("bf16", "fp16"):
    c = R.shrink(_first(lambda c: c["kind"] == "fp32_rows" and c["dtype"] == dtype and c["dropout_p"] == 0.0 and not c["decode"]))
    t, ref, base = _made(c)
    wrong = _recompute(c, t, ref, bias=R.mask4(c, t["mask"].to(R.DTYPES[dtype])))
    worst = max(_rel(g, r) / _rel(b, r) for g, b, r in zip(wrong, base["grads"], ref["grads"]))
    print(f"[ratio] fp32 bias ~ N(0, {c['bias_scale']}) rounded to {dtype}: worst err / baseline {worst:.2f}")
    assert C < worst < 4 * C, worst


# ----------------------------------------------------------------------------- the rule that answers the fault
@pytest.mark.parametrize("seed", [s for s in R.SWEEP_SEEDS if CASES[s]["aten_may_serve"]])
def test_an_fp32_bias_next_to_16_bit_queries_never_reaches_aten(seed, monkeypatch):
  """``attention_backward`` on the storage-dtype tensors of every case aten could serve: an fp32 bias (``finfo(float32).min`` padding included, which a
  conversion to 16 bits turns into -inf) takes the recompute and refuses ``force="aten"``; every other mask still tries aten first."""
  c = R.shrink(CASES[seed])
  t, ref, _ = _made(c)
  tried = []
  monkeypatch.setattr(bw, "_aten_unsupported", {})
  monkeypatch.setattr(bw, "_aten_efficient_backward", lambda *a: tried.append(a[8]) or bw._chunked_recompute_backward(*a))  # (no such op on a CPU: note the try)
  args = (t["go"], t["q"], t["k"], t["v"], ref["o"].to(t["q"].dtype), ref["lse"].float())
  kw = dict(causal=c["causal"], scale=c["D"] ** -0.5, attn_bias=R.mask4(c, t["mask"]), want_bias_grad=c["bias_grad"])
  got = bw.attention_backward(*args, **kw)
  fp32 = t["mask"] is not None and t["mask"].dtype == torch.float32
  assert fp32 == (R.mask_form(c)[0] in ("fp32", "fp32_min")) and len(tried) == (0 if fp32 else 1)
  assert all(b is None or b.dtype == t["q"].dtype for b in tried)  # (what reaches aten is in the queries' dtype already: nothing is rounded on the way)
  if fp32:
    with pytest.raises(NotImplementedError, match="bias"):
      bw.attention_backward(*args, **kw, force="aten")
    want = bw.attention_backward(*args, **kw, force="recompute")
    assert all(torch.equal(a, b) for a, b in zip(got[:3], want[:3])) and (got[3] is None or (got[3].dtype == torch.float32 and torch.equal(got[3], want[3])))


def padded_rows_case(dtype, nq, nkv, D, value, device="cpu"):
  """The padding mask of model code (tests/model_values.py ``hf_mask``) as an fp32 ``[2, 1, Nq, Nkv]`` mask: sequence 1 is left-padded — its first Nkv // 3 keys
  carry ``value`` for every row, and its first 3 rows (padding tokens themselves) carry it on EVERY key: SDPA-math rows, which the forward computes as the
  softmax of what fp32 leaves of ``S + value`` (at finfo(float32).min: uniform attention).  -> (case, tensors) in backward_dense_ref's vocabulary."""
  c = dict(seed=0, kind="padded_rows", B=2, heads=(4, 2), Nq=nq, Nkv=nkv, D=D, dtype=dtype, causal=False, bias_grad=False, dropout_p=0.0)
  gen = torch.Generator().manual_seed(nq + nkv)
  t = {n: torch.randn(2, h, rows, D, generator=gen).to(R.DTYPES[dtype]).to(device) for n, h, rows in (("q", 4, nq), ("k", 2, nkv), ("v", 2, nkv), ("go", 4, nq))}
  mask = torch.zeros(2, 1, nq, nkv)
  mask[1, 0, :, :nkv // 3] = value
  mask[1, 0, :3] = value
  t.update(mask=mask.to(device), dropout=None)
  return c, t


@pytest.mark.parametrize("value", [torch.finfo(torch.float32).min, -1e4])
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_rows_masked_on_every_key_by_a_finite_value_get_the_gradient_of_what_the_forward_computed(dtype, value):
  """The backward on what the kernel hands it — O in the storage dtype, the LSE in fp32 (here: float32 math) — for rows whose LSE sits at the mask value: at
  finfo(float32).min an fp32 LSE has absorbed the log of the row's sum, and exp(S - LSE) would be 1 per key instead of 1 / Nkv (dq of such a row Nkv times
  too large).  Every gradient, and dq of those rows alone, against float64 by the comparator."""
  c, t = padded_rows_case(dtype, 12, 37, 16, value)
  ref, base, f32 = R.reference(c, t), R.baseline(c, t), R.reference(c, t, math=torch.float32)
  assert bool((f32["lse"][1, :, :3].abs() >= bw.LSE_COARSE).all()) and bool((f32["lse"][0].abs() < 10).all())
  got = bw.attention_backward(t["go"], t["q"], t["k"], t["v"], f32["o"].to(t["q"].dtype), f32["lse"], causal=False, scale=c["D"] ** -0.5, attn_bias=t["mask"])
  _compare(f"padded rows {dtype}", got[:3], base["grads"], ref["grads"])
  _compare(f"padded rows {dtype}: their dq", [got[0][1, :, :3]], [base["grads"][0][1, :, :3]], [ref["grads"][0][1, :, :3]], names=("dq",))
  assert ref["grads"][0][1, :, :3].norm().item() > 0.0
  if value < -1e30:  # ... and with the LSE the kernel writes for a saturated row: -2^100 / l (csrc/ffpa_common.h ``row_lse``)
    sat = f32["lse"].clone()
    sat[1, :, :3] = -(2.0 ** 100) / c["Nkv"]
    got = bw.attention_backward(t["go"], t["q"], t["k"], t["v"], f32["o"].to(t["q"].dtype), sat, causal=False, scale=c["D"] ** -0.5, attn_bias=t["mask"])
    _compare(f"padded rows {dtype}, saturated LSE", got[:3], base["grads"], ref["grads"])


# ----------------------------------------------------------------------------- the keep mask against the oracle's Philox
@pytest.mark.parametrize("offset", [0, 5, 4 * ((1 << 33) + 5) + 2])
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_keep_mask_matches_the_oracle_philox_at_batch_and_head_terms(p, offset):
  """300 sampled elements of a B 2, Hq 4, Nq 130, Nkv 777 call — batch and head terms, offsets inside a Philox quad, a 62-bit seed: word ``(e + offset) & 3`` of
  the oracle's block ``(e + offset) >> 2``, ``u = (word + 1) 2^-32`` in fp32, kept iff ``u > p``."""
  c = dict(B=2, heads=(4, 2), Nq=130, Nkv=777)
  seed = (1 << 61) + 0x1234_5678_9ABC_DEF
  assert seed.bit_length() == 62
  idx = R.element_index(c, "cpu")
  keep = dropout_keep_mask(seed, offset, idx, p)
  rnd = random.Random(11)
  picks = [(rnd.randrange(2), rnd.randrange(4), rnd.randrange(130), rnd.randrange(777)) for _ in range(296)] + [(1, 3, 129, 776), (1, 0, 0, 0), (0, 3, 129, 776), (1, 2, 64, 3)]
  for b, h, r, j in picks:
    e = ((b * 4 + h) * 130 + r) * 777 + j
    assert int(idx[b, h, r, j]) == e
    w = fo.philox4x32_10(seed, (e + offset) >> 2)[(e + offset) & 3]
    assert bool(keep[b, h, r, j]) == bool((np.float32(w) + np.float32(1.0)) * np.float32(2.3283064365386963e-10) > np.float32(p)), (b, h, r, j)
  assert any(b == 1 for b, *_ in picks) and abs(keep.float().mean().item() - (1 - p)) < 4 * (p * (1 - p) / keep.numel()) ** 0.5
