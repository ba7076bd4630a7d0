"""The KV-cache family sweep's generator and float64 reference (tests/kvcache_family_ref.py), judged without a GPU and on the reference alone: the coverage of the
committed seeds; the family reference against the per-feature restatements the suites already use (``kvcache_ref.attend``, ``kvcache_window_ref.attend``,
``kvcache_softcap_ref.attend``, ``tree_ref.attend_tree`` and ``brute_force``, ``kvcache_varlen_ref.reference``) on the sweep's own cases, to 1e-12; the conditions
that keep a case from being vacuous (rows that see a key; a window, a cap, a tree mask that moves the output by more than 10 allowances in at least half the
rows); the model-like cases' family properties at the launch's tile; and ``kvcache_ref.check`` shown to reject the family reference broken the way such kernels
break.  The conditions are asserted here on the cases a CPU computes in about a second each (``_cheap``) and on EVERY case by tests/test_kvcache_family_gpu.py."""

import collections

import pytest
import torch

import kvcache_family_ref as F
import kvcache_ref as R
import kvcache_softcap_ref as S
import kvcache_varlen_ref as V
import kvcache_window_ref as W
import model_values as mv
import tree_ref

CASES = [F.draw_case(s) for s in F.SWEEP_SEEDS]


def _cost(c):
  return max(F.effective_lens(c)) * sum(c["qlens"]) * c["heads"][0] * c["D"]


def _cheap(c):
  return _cost(c) <= 2e9 and c["B"] * c["capacity"] * c["heads"][1] * c["D"] <= 3e7


_MADE: dict = {}


def _made(c):
  """A case's CPU tensors, its units and reference: made once and shared (nothing writes to them)."""
  if c["seed"] not in _MADE:
    t = F.materialize(c)
    us, caches = F.units(c, t)
    _MADE[c["seed"]] = (t, us, caches) + F.attend_units(c, us)
  return _MADE[c["seed"]]


# ----------------------------------------------------------------------------- the generator
def test_the_seed_list_covers_every_axis():
  assert F.SWEEP_SEEDS == tuple(range(80)) and len(F.CALLS) == 10
  assert {F.PUBLIC[call] for call in F.CALLS} == {"ffpa_attn_with_kvcache", "ffpa_attn_with_kvcache_window", "ffpa_attn_with_kvcache_softcap", "ffpa_attn_with_kvcache_tree",
                                                  "ffpa_attn_with_kvcache_cascade", "ffpa_attn_varlen_with_kvcache"}
  count = lambda key, cases=CASES: collections.Counter(c[key] for c in cases)
  for call in F.CALLS:
    mine = [c for c in CASES if c["call"] == call]
    assert len(mine) == 8
    assert set(count("num_splits", mine)) == set(F.SPLITS), call
    assert set(count("dtype", mine)) == {"bf16", "fp16"}, call
    assert set(count("stream", mine)) == set(F.STREAMS), call
    want_pages = {0} if call == "varlen_packed" else set(F.PAGES[:3]) if call == "varlen_paged" else set(F.PAGES)
    assert set(count("page", mine)) == want_pages, call
    # the append: absent, as many rows as tokens, 1 or 3 rows under other token counts (a ragged call appends its tokens' rows), with rotary (not the tree call)
    assert {"none", "same", "few"} <= set(count("append", mine)), call
    assert call == "tree" or any(c["rotary_dim"] for c in mine), call
    assert sum(c["model"] is not None for c in mine) == 2, call
  assert {c["call"] for c in CASES if c["page"]} >= set(F.CALLS) - {"varlen_packed"} and {c["call"] for c in CASES if not c["page"]} >= set(F.CALLS) - {"varlen_paged"}
  assert set(count("interleaved", [c for c in CASES if c["rotary_dim"]])) == {False, True}
  few = {(c["snew"][0], c["Sq"]) for c in CASES if c["append"] == "few" and not c["ragged"]}
  assert {n for n, _ in few} == {1, 3} and any(n != sq for n, sq in few)
  assert set(count("heads")) == set(F.HEADS) and set(count("layout")) == set(R.POOL_LAYOUTS)
  assert set(count("table_layout", [c for c in CASES if c["page"]])) == set(R.TABLE_LAYOUTS) and set(count("lens_strided")) == {False, True}
  assert set(count("fused_qkv")) == {False, True} and set(count("bad_unused_ids", [c for c in CASES if c["page"]])) == {False, True}
  assert set(count("head_dim_class")) == set(R.PAGED_HEAD_DIM_CLASSES)
  assert any(c["D"] != c["head_dim_class"] for c in CASES) and all(c["D"] % 8 == 0 and c["head_dim_class"] - 64 < c["D"] <= c["head_dim_class"] or c["D"] < 128 for c in CASES)
  assert all({c["dtype"] for c in CASES if (c["head_dim_class"] <= 512) == small} == {"bf16", "fp16"} for small in (True, False))
  # model values: one case in four, every family at least twice, every staircase step, both directions
  model = [c for c in CASES if c["model"]]
  assert len(model) == len(CASES) // 4
  fams = collections.Counter(mv.VARIANTS[c["model"]][0] for c in model)
  assert set(fams) == {"outliers", "sink", "peaked", "staircase_up", "staircase_down", "large_logits"} and min(fams.values()) >= 2, fams
  assert {mv.VARIANTS[c["model"]][1]["step"] for c in model if "staircase" in c["model"]} == set(mv.STAIR_STEPS)
  assert all(c["model"] in F.MODEL_CAP for c in model if c["capped"]) and all(c["model"] in F.MODEL_WINDOW for c in model if c["windowed"] and not c["capped"])
  assert all(not c["rotary_dim"] for c in model) and {c["num_splits"] for c in model} == set(F.SPLITS)
  # windows: every kind under every windowed call; span 0, the identity (at least the longest sequence), a non-causal pair with right > 0
  for call in F.CALLS:
    mine = [c for c in CASES if c["call"] == call and c["windowed"]]
    assert not mine or set(count("window_kind", mine)) >= set(F.WINDOW_KINDS), call
  for c in CASES:
    if c["windowed"]:
      left, right = c["window"]
      assert {"span0": left == 0, "identity": left >= max(F.effective_lens(c)) and right == -1, "noncausal": right > 0 and left >= 1 and not c["causal"],
              "short": left >= 1, "quarter": left >= 1, "tiles": left == 2 * F.block_keys(c) + 5}[c["window_kind"]], c
    else:
      assert c["window"] == (-1, -1)
  import test_kvcache_softcap_gpu as SG  # (its constants only: nothing of it runs here)

  assert (F.CAPS, F.FACTOR) == (SG.CAPS, SG.FACTOR)
  caps = [c for c in CASES if c["capped"]]
  assert set(count("softcap", caps)) == set(F.CAPS) and all({c["softcap"] for c in caps if c["call"] == call} == set(F.CAPS) for call in F.CALLS if "softcap" in call)
  trees = [c for c in CASES if c["tree"]]
  assert set(count("mask_kind", trees)) == set(tree_ref.MASK_KINDS) and set(count("per_sequence", trees)) == {False, True}
  assert max(c["Sq"] for c in trees) == 64 and all(1 <= c["Sq"] <= 64 for c in trees)
  assert [c["seed"] for c in trees if not c["tree_matters"]] == [c["seed"] for c in trees if c["mask_kind"] == "tril"] and sum(c["tree_matters"] for c in trees) == 7
  assert all(c["tree_matters"] and "staircase_up" in c["model"] for c in trees if c["model"])  # (a tree word hiding the largest score, on model values)
  # ragged batches: a chunk of 65 ... 300 tokens (but in the long cases), 2 ... 5-token sequences, one-token decodes, empty sequences
  for c in CASES:
    if c["ragged"] and not c["model"]:
      assert 0 in c["qlens"] and 1 in c["qlens"] and any(2 <= n <= 5 for n in c["qlens"]), c["qlens"]
      assert c["long"] or any(65 <= n <= 300 for n in c["qlens"]), c["qlens"]
  assert any(65 <= c["Sq"] <= 300 for c in CASES if not c["ragged"])
  # lengths: the edges, about 1400 keys at the most, about one case in five at 2500 ... 6000
  edge = collections.Counter()
  for c in CASES:
    unit, cap = c["page"] or 64, c["capacity"]
    for n in c["lens"]:
      for name, hit in (("0", n == 0), ("negative", n < 0), ("1", n == 1), ("unit - 1", n == unit - 1), ("unit", n == unit), ("unit + 1", n == unit + 1),
                        ("capacity", n == cap), ("capacity + 5", n == cap + 5)):
        edge[name] += hit
  assert all(edge[name] >= 1 for name in ("0", "negative", "1", "unit - 1", "unit", "unit + 1", "capacity", "capacity + 5")), edge
  longest = [max(F.effective_lens(c)) for c in CASES]
  assert sum(2500 <= n <= 6000 for n in longest) >= len(CASES) // 6 and all(n <= 6000 for n in longest), sorted(longest)
  assert all(n <= 1400 + 2 * 256 for n, c in zip(longest, CASES) if not c["long"])
  # the cascade's contract: every sequence holds the shared prefix (a whole number of pages), its suffix the step's tokens
  for c in CASES:
    if c["cascade"]:
      P = c["shared_prefix_len"]
      assert 0 < P < c["capacity"] and (not c["page"] or P % c["page"] == 0) and all(n >= P + c["Sq"] for n in F.effective_lens(c)), c


def test_no_case_is_vacuous():
  """At least 90 % of the sweep's query rows see a key, and every case has a row that does — but the deliberate all-empty edge case, listed by seed."""
  seen, rows = zip(*(F.visible_rows(c) for c in CASES))
  assert sum(seen) >= 0.9 * sum(rows), (sum(seen), sum(rows))
  assert tuple(c["seed"] for c, s in zip(CASES, seen) if s == 0) == F.ALL_EMPTY_SEEDS
  assert all(sum(c["qlens"]) > 0 for c in CASES)


def test_kernel_names():
  assert F.kernel_of(F.draw_case(0)).startswith("ffpa_fwd_m16_") and F.kernel_of(F.draw_case(0)).endswith("_kernel<" + F.draw_case(0)["dtype"] + ", ")
  stems = {F.kernel_of(c).split("<")[0] for c in CASES}
  assert stems == {f"ffpa_fwd_m16_{where}{kind}_kernel" for where in ("paged", "varlen") for kind in ("", "_window", "_softcap", "_tree")}
  assert {F.block_keys(c) for c in CASES} == {64, 32, 128} and all(not c["page"] and c["head_dim_class"] in (256, 320) for c in CASES if F.block_keys(c) == 128)


# ----------------------------------------------------------------------------- the reference
def _older(c, t, us, caches):
  """``(o [T, Hq, D], lse [T, Hq])`` of a case by the restatement its own suite uses, on the caches after the append."""
  kview, vview = caches[:2]
  eff = F.effective_lens(c)
  if c["ragged"]:
    vt = dict(q=t["q"], k=t["k"], v=t["v"], cu=t["cu"], lens=torch.tensor(c["lens"]), table=t["table"], k_cache=t["k_cache"], v_cache=t["v_cache"], cos=t["cos"],
              sin=t["sin"], seqs=c["qlens"], capacity=c["capacity"], dtype=c["dtype"])
    (o, lse, _, _), _, _, _, lens = V.reference(vt, append_kv=t["k"] is not None, rotary=t["cos"] is not None, interleaved=c["interleaved"], causal=c["causal"],
                                                window=c["window"], softcap=c["softcap"])
    assert lens == eff
    return o[0], lse[0].t()
  q = torch.stack([u[0] for u in us])  # (the rotated copy that attends)
  if c["tree"]:
    o, lse, _, _ = tree_ref.attend_tree(q, kview, vview, eff, t["table"], t["tree_mask"])
  elif c["capped"]:
    o, lse, _, _ = S.attend(q, kview, vview, eff, t["table"], c["window"], c["causal"], softcap=c["softcap"])
  elif c["windowed"]:
    o, lse, _, _ = W.attend(q, kview, vview, eff, t["table"], c["window"], c["causal"])
  else:  # (the cascade is the plain call over the whole cache: its passes and merge are how, not what)
    o, lse, _, _ = R.attend(q, kview, vview, eff, t["table"], c["causal"])
  return o.flatten(0, 1), lse.permute(0, 2, 1).flatten(0, 1)


@pytest.mark.parametrize("call", F.CALLS)
def test_the_family_reference_is_the_per_feature_reference(call):
  """Every cheap case of the call, and at least three, one of them with an append."""
  mine = [c for c in CASES if c["call"] == call and _cheap(c)]
  assert len(mine) >= 3 and any(c["append"] != "none" for c in mine) and (call == "tree" or any(c["rotary_dim"] for c in mine)), [c["seed"] for c in mine]
  for c in mine:
    t, us, caches, (o, lse, pmax, p2sum), vstat = _made(c)
    T, hq = sum(c["qlens"]), c["heads"][0]
    assert o.shape == (T, 1, hq, c["D"]) and lse.shape == pmax.shape == p2sum.shape == (T, hq, 1)
    want_o, want_lse = _older(c, t, us, caches)
    assert torch.isfinite(o).all() and torch.allclose(o[:, 0], want_o, atol=1e-12, rtol=1e-12), (c["seed"], (o[:, 0] - want_o).abs().max())
    assert torch.equal(torch.isneginf(lse[:, :, 0]), torch.isneginf(want_lse)), c["seed"]
    fin = torch.isfinite(want_lse)
    assert torch.allclose(lse[:, :, 0][fin], want_lse[fin], atol=1e-12, rtol=1e-12), c["seed"]
    assert (o[:, 0][~fin] == 0).all() and (pmax[:, :, 0][~fin] == 0).all() and ((pmax > 0) & (pmax <= 1) | ~fin[:, :, None]).all()
    assert vstat[0] >= vstat[1] > 0


def test_the_tree_reference_is_the_brute_force():
  c = min((c for c in CASES if c["tree"] and not c["model"]), key=_cost)
  t, us, caches, (o, lse, _, _), _ = _made(c)
  want_o, want_lse = tree_ref.brute_force(torch.stack([u[0] for u in us]), caches[0], caches[1], F.effective_lens(c), t["table"], t["tree_mask"])
  assert torch.allclose(o[:, 0], want_o.flatten(0, 1), atol=1e-12, rtol=1e-12)
  fin = torch.isfinite(want_lse)
  assert torch.allclose(lse[:, :, 0].t().reshape(want_lse.shape[1], c["B"], c["Sq"]).permute(1, 0, 2)[fin], want_lse[fin], atol=1e-12, rtol=1e-12)


def _bits(x):
  return x.view(torch.int16)


@pytest.mark.parametrize("call", F.CALLS)
def test_a_case_materializes_on_the_cpu_and_appends_where_the_contract_says(call):
  """Unused pages, rows behind a length and everything outside the views hold NaN before the call; after it, row i of sequence b sits at ``max(len_b, 0) + i`` —
  rows at or past the capacity dropped — and nothing else of the storage has changed."""
  c = min((c for c in CASES if c["call"] == call and c["append"] != "none" and not c["rotary_dim"] and _cheap(c)), key=_cost)
  t, us, (kview, vview, ks, vs, rotated), _, _ = _made(c)
  page, cap, n = t["k_cache"].size(1), c["capacity"], t["k_cache"].size(0)
  where = lambda b, p: (b if t["table"] is None else min(max(int(t["table"][b, p // page]), 0), n - 1), p % page)
  live = torch.zeros(t["k_cache"].shape[:2], dtype=torch.bool)
  for b, ln in enumerate(c["lens"]):
    for p in range(min(max(ln, 0), cap)):
      live[where(b, p)] = True
  for view, storage in ((t["k_cache"], t["k_storage"]), (t["v_cache"], t["v_storage"])):
    assert torch.isnan(view[~live]).all() and torch.isfinite(view[live]).all()
  want_k, want_v = t["k_storage"].clone(), (t["v_storage"].clone() if t["v_storage"] is not t["k_storage"] else None)
  wk = R.reviewed(t["k_cache"], t["k_storage"], want_k)
  wv = R.reviewed(t["v_cache"], t["v_storage"], want_k if want_v is None else want_v)
  start = landed = 0
  for b, ln in enumerate(c["lens"]):
    for i in range(c["snew"][b] or 0):
      p = max(ln, 0) + i
      if p < cap:
        wk[where(b, p)], wv[where(b, p)] = (t["k"][start + i], t["v"][start + i]) if c["ragged"] else (t["k"][b, i], t["v"][b, i])
        landed += 1
    start += c["qlens"][b] if c["ragged"] else 0
  assert landed > 0 and not rotated
  assert torch.equal(_bits(ks), _bits(want_k)) and (want_v is None or torch.equal(_bits(vs), _bits(want_v)))


# ----------------------------------------------------------------------------- the conditions
def _feature_cases():
  return [c for c in CASES if F.features_off(c)]


def test_the_feature_of_a_case_moves_its_output():
  """A window hides something, a cap bends something, a tree mask hides something: against the same case with the feature off, the float64 outputs differ by
  more than 10 allowances in at least half the non-empty rows (tests/test_kvcache_softcap_gpu.py's ``_cap_matters`` rule: 0.5 and 10 x).  Excepted by design: the
  ``identity`` window kind, a cap under span 0 (a row sees one key) and the ``tril`` mask kind, which is plain causal (kvcache_family_ref.features_off).  A
  window call with a cap answers for both, one at a time; EVERY other tree case answers for its mask."""
  cases = [c for c in _feature_cases() if _cheap(c)]
  names = [name for c in cases for name, _ in F.features_off(c)]
  assert names.count("window") >= 10 and names.count("cap") >= 8 and names.count("tree mask") == 7, names
  for c in cases:
    t, us, _, ref, vstat = _made(c)
    for name, off in F.features_off(c):
      t_off = dict(t, tree_mask=F.case_mask(off)) if c["tree"] else t
      other, _, _ = F.reference(off, t_off)
      share = F.moved_share(c, ref, other, vstat)
      print(f"seed {c['seed']} {c['call']} window {c['window']} cap {c['softcap']}: the {name} moves {share:.0%} of the non-empty rows")
      assert share >= 0.5, (c["seed"], c["call"], name, c["window"], c["softcap"], share)


def test_an_identity_window_is_the_plain_call():
  cases = [c for c in CASES if c["window_kind"] == "identity" and _cheap(c)]
  assert len(cases) >= 3
  for c in cases:
    t, us, _, ref, _ = _made(c)
    other, _, _ = F.reference(dict(c, window=(-1, -1)), t)
    assert all(torch.equal(a, b) for a, b in zip(ref, other)), c["seed"]


def test_model_like_cases_show_their_family_property():
  """One case in four lays a tests/model_values.py family out as cache rows; what the family promises is asserted on the float64 scores of the rows the call
  computes, over the keys each row sees, and a staircase crosses the tile boundaries of the launch's own ``block_keys``."""
  model = [c for c in CASES if c["model"]]
  for c in model:
    t, us, _, ref, _ = _made(c)
    assert all(u[1].size(0) in F.MODEL_LENS for u in us), c["seed"]
    fig = F.assert_model_property(c, us)
    print(f"seed {c['seed']} {c['call']} {c['model']} D{c['D']} block_keys {F.block_keys(c)}: {fig}")
  assert {F.block_keys(c) for c in model if "staircase" in c["model"]} >= {64, 32}


# ----------------------------------------------------------------------------- the checker bites
_APPLIES = {"window_left": lambda c: c["windowed"] and c["window_kind"] in ("span0", "short", "noncausal"),
            "window_right": lambda c: c["windowed"] and c["window_kind"] in ("span0", "short", "noncausal", "quarter") and c["Sq"] > 1,
            "cap_after_mask": lambda c: c["capped"] and (c["causal"] or c["windowed"]),
            "tree_shift": lambda c: c["tree"] and c["tree_matters"] and c["mask_kind"] != "ones",
            "align": lambda c: not c["tree"] and (c["causal"] or c["windowed"]) and c["window_kind"] != "identity",
            "drop_last_tile": lambda c: not c["windowed"]}


@pytest.mark.parametrize("mutation", F.MUTATIONS)
def test_checker_rejects_a_subtly_wrong_reference(mutation):
  """The family reference's own output rounded to the case's dtype passes ``kvcache_ref.check``; the same reference with the window off by one key on either side,
  the cap applied after the mask, the tree word shifted by one bit, the bottom-right alignment off by one or the last tile dropped does not — on sweep cases."""
  cases = sorted((c for c in CASES if _APPLIES[mutation](c) and _cheap(c) and not c["model"]), key=_cost)
  assert cases, mutation
  caught = 0
  for c in cases[:12]:
    if caught:
      break
    t, us, _, ref, vstat = _made(c)
    dtype = R.TORCH_DTYPE[c["dtype"]]
    assert R.check(ref[0].to(dtype), ref[1].float(), ref, v=vstat, dtype=c["dtype"], name="intact") <= 1.0
    bad, _, _ = F.reference(c, t, mut=mutation)
    try:
      R.check(bad[0].to(dtype), bad[1].float(), ref, v=vstat, dtype=c["dtype"], name=mutation)
    except AssertionError as e:
      assert "max err" in str(e) or "LSE" in str(e) or "not 0" in str(e), e
      caught += 1
  assert caught >= 1, (mutation, [c["seed"] for c in cases[:12]])
