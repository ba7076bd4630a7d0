"""The family sweep's generator and float64 reference (tests/kvcache_mla_family_ref.py), checked without a GPU and on the reference alone: the coverage conditions
of the committed seeds; the family reference against the per-call references the suites already use (``kvcache_ref.attend``, ``tree_ref.attend_tree``,
``kvcache_mla_sparse_ref.reference``, the cascade's plan ``kvcache_mla_cascade_ref.plan`` with a float64 merge, ``pool.double() * kv_scale``) on one small case per
call, to 1e-12; the appended rows against a row-by-row restatement of the append; the model-like cases' family properties; and ``kvcache_ref.check`` shown to
reject the family reference's own output broken the way such kernels break, at 100 and at 4000 keys."""

import collections

import pytest
import torch

import kvcache_mla_cascade_ref as CR
import kvcache_mla_family_ref as F
import kvcache_mla_sparse_ref as SR
import kvcache_ref as R
import tree_ref

CASES = [F.draw_case(s) for s in F.SWEEP_SEEDS]


def _cost(c):
  keys = max(F.counts_of(c)) if c["sparse"] else max(F.effective_lens(c))
  return (c["model"] is not None, c["long"], keys * sum(c["qlens"]) * c["heads"][0])


SMALL = {call: min((c for c in CASES if c["call"] == call and (c["append"] != "none" or c["sparse"] and not c["ds"])), key=_cost) for call in F.CALLS}


# ----------------------------------------------------------------------------- the generator
def test_the_seed_list_covers_every_axis():
  assert F.SWEEP_SEEDS == tuple(range(104)) and len(F.CALLS) == 13
  count = lambda key, cases=CASES: collections.Counter(c[key] for c in cases)
  dense, sparse = [c for c in CASES if not c["sparse"]], [c for c in CASES if c["sparse"]]
  assert all(count("call")[call] >= 8 for call in F.CALLS), count("call")
  assert set(count("dtype")) == {"bf16", "fp16"} and all(c["dtype"] == "bf16" for c in CASES if c["ds"])
  assert set(count("heads")) == set(F.HEADS), count("heads")
  uniform = [c for c in CASES if not c["ragged"] and not c["tree"] and not c["sparse"]]
  assert {c["Sq"] for c in uniform} == set(F.UNIFORM_SQ) and {c["T"] // c["B"] for c in sparse} == set(F.UNIFORM_SQ)
  trees = [c for c in CASES if c["tree"]]
  assert max(max(c["qlens"]) for c in trees) == 64 and min(max(c["qlens"]) for c in trees) == 1
  for c in CASES:
    if c["ragged"] and not c["model"]:  # a ragged batch mixes an empty sequence, a one-token decode and a chunk of 40 ... 70 tokens
      assert 0 in c["qlens"] and 1 in c["qlens"] and any(40 <= n <= 70 for n in c["qlens"]), c["qlens"]
    assert not c["tree"] or max(c["qlens"]) <= 64
  assert set(count("page", dense)) == set(F.PAGES) and set(count("form", sparse)) == set(F.SPARSE_FORMS)
  assert all(c["page"] for c in CASES if c["cascade"])
  assert set(count("table_layout", [c for c in dense if c["page"]])) == set(R.TABLE_LAYOUTS)
  assert set(count("lens_strided")) == {False, True} and set(count("pad")) == {0, 16}
  assert set(count("num_splits")) == set(F.SPLITS) and set(count("stream")) == set(F.STREAMS)
  assert set(count("causal", [c for c in dense if not c["tree"]])) == {False, True}
  assert set(count("kv_scale", [c for c in CASES if c["fp8"]])) == set(F.KV_SCALES)
  assert set(count("mask_kind", trees)) == set(tree_ref.MASK_KINDS) and set(count("per_sequence", trees)) == {False, True}
  # the append: absent, as many rows as tokens, 1 and 3 rows under other token counts, a length at the capacity's edge; the 656-byte rows stored by slot
  assert set(count("append", dense)) == set(F.APPENDS) and set(count("append", [c for c in CASES if c["ds"]])) == {"none", "store"}
  few = {(c["snew"][0], c["Sq"]) for c in dense if c["append"] == "few" and not c["ragged"]}  # (a ragged call appends its tokens' rows, whatever the kind)
  assert {n for n, _ in few} == {1, 3} and any(n != sq for n, sq in few)
  assert any(n == c["capacity"] - 1 and s for c in dense if c["append"] == "edge" for n, s in zip(c["lens"], c["snew"]))
  for call in F.CALLS:
    mine = [c for c in CASES if c["call"] == call]
    assert any(c["num_splits"] > 1 for c in mine), call
    if "_sparse" not in call or call.endswith("_ds"):
      assert any(c["append"] != "none" for c in mine), call
  # the cascade: one group and several with an empty one, host and device prefixes, a stated prefix longer than the shortest sequence
  cas = [c for c in CASES if c["cascade"]]
  assert any(len(c["group_sizes"]) == 1 for c in cas) and any(0 in c["group_sizes"] for c in cas)
  assert set(count("prefix_on_device", cas)) == {False, True}
  stated = lambda c: max(c["stated_prefix"]) if c["prefix_on_device"] else c["stated_prefix"]
  assert any(0 < min(F.effective_lens(c)) < stated(c) for c in cas)
  # lengths (counts, for the index lists): the edges, about 1400 keys at the most, one case in five at 2500 ... 6000
  edge = collections.Counter()
  for c in CASES:
    unit, cap = c["page"] or 64, c["capacity"]
    for n in (c["counts"] if c["sparse"] else c["lens"]):
      for name, hit in (("0", n == 0), ("negative", n < 0), ("1", n == 1), ("31", n == 31), ("32", n == 32), ("33", n == 33), ("page - 1", n == unit - 1),
                        ("page + 1", n == unit + 1), ("capacity", n == cap), ("capacity + 5", n == cap + 5)):
        edge[name] += hit
  assert all(edge[name] >= 1 for name in ("0", "negative", "1", "31", "32", "33", "page - 1", "page + 1", "capacity", "capacity + 5")), edge
  longest = [max(F.counts_of(c)) if c["sparse"] else max(F.effective_lens(c)) for c in CASES]
  assert sum(2500 <= n <= 6000 for n in longest) >= len(CASES) // 5 and all(n <= 6000 for n in longest)
  assert all(n <= 1400 + 2 * 256 for n, c in zip(longest, CASES) if not c["long"])  # (a reach below 1400 keys, rounded up to whole pages, and one page more)
  # index lists: every filler behind a count, duplicates in front of it
  behind, dup = set(), 0
  for c in sparse:
    for row, n in zip(c["indices"], F.counts_of(c)):
      behind |= set(row[n:])
      dup += len(set(row[:n])) < n
      assert all(0 <= s < c["num_rows"] for s in row[:n]) and len(row) == c["topk"]
  assert behind == set(F.BEHIND) and dup >= 8
  assert any(c["counts_none"] for c in sparse) and any(not c["counts_none"] for c in sparse)
  # data: one seed in four takes a model_values family
  assert sum(c["model"] is not None for c in CASES) == len(CASES) // 4 and all((c["model"] is not None) == (c["seed"] % 4 == 1) for c in CASES)
  # rows per (sequence, latent head)
  classes = collections.Counter(name for c in CASES for name in F.row_classes(c))
  assert all(classes[name] >= 3 for name in ("<16", "16-63", "64", "65-127", ">=128")), classes
  # at most a quarter of the query rows see no key (tests/test_tree_ref.py's cap), and no case has all its rows empty
  seen, rows = zip(*(F.visible_rows(c) for c in CASES))
  assert sum(seen) >= 0.75 * sum(rows), (sum(seen), sum(rows))
  assert all(s > 0 for s in seen), [c["seed"] for c, s in zip(CASES, seen) if s == 0]


def test_kernel_names():
  assert F.kernel_of(F.draw_case(0)) == "ffpa_fwd_m16_mla_kernel<bf16, 576, dv=512"
  names = {F.kernel_of(c).split("<")[0] for c in CASES}
  assert names == {"ffpa_fwd_m16_mla" + k + "_kernel" for k in ("", "_fp8", "_tree", "_tree_fp8", "_sparse", "_sparse_fp8", "_sparse_ds")}


# ----------------------------------------------------------------------------- the reference
def _merge(o_a, l_a, o_b, l_b):
  """Two (O, LSE) states over disjoint keys -> the state over both, in float64; l [.., Hq, Sq] against o [.., Sq, Hq, dv]."""
  l = torch.logaddexp(l_a, l_b)
  w = lambda x: torch.where(torch.isneginf(l), torch.zeros_like(l), torch.exp(x - torch.where(torch.isneginf(l), torch.zeros_like(l), l))).transpose(-1, -2)[..., None]
  return o_a * w(l_a) + o_b * w(l_b), l


def _per_call_reference(c, t, storage):
  """``(o [T, Hq, dv], lse [T, Hq])`` of a case by the reference its own suite uses, on the dequantised post-append pool."""
  view = R.reviewed(t["view"], t["storage"], storage)
  pool = F.decode(c, view)
  if c["sparse"]:
    o, lse, _, _ = SR.reference(t["q"], pool, t["indices"], c["counts"], c["scale"], F.DV)
    return o[:, 0], lse[:, :, 0]
  table, lens, outs, start = t["table"], F.effective_lens(c), [], 0
  if c["cascade"]:
    cu_g = t["cu_group_seqs"]
    _, len_pre, table_pre, table_suf, len_suf = CR.plan(torch.tensor(lens), table, cu_g, t["shared_prefix_len"], c["page"], c["Sq"], c["causal"], c["capacity"])
    group_of = [g for g, n in enumerate(c["group_sizes"]) for _ in range(n)]
  for b, n_tok in enumerate(c["qlens"]):
    q = (t["q"][start:start + n_tok] if c["ragged"] else t["q"][b])[None]
    start += n_tok
    slab = pool[b:b + 1] if table is None else pool
    row = None if table is None else table[b:b + 1]
    if c["tree"]:
      m = t["tree_mask"] if t["tree_mask"].dim() == 2 else t["tree_mask"][b]
      o, lse, _, _ = tree_ref.attend_tree(q, slab, slab, [lens[b]], row, m[:n_tok, :n_tok], c["scale"])
    elif c["cascade"]:
      g = group_of[b]
      o_p, l_p, _, _ = R.attend(q, slab, slab, [int(len_pre[g])], table_pre[g:g + 1], False, c["scale"])
      o_s, l_s, _, _ = R.attend(q, slab, slab, [int(len_suf[b])], table_suf[b:b + 1], c["causal"], c["scale"])
      o, lse = _merge(o_p, l_p, o_s, l_s)
    else:
      o, lse, _, _ = R.attend(q, slab, slab, [lens[b]], row, c["causal"], c["scale"])
    outs.append((o[0, ..., :F.DV], lse[0].t()))
  return torch.cat([o for o, _ in outs]), torch.cat([l for _, l in outs])


@pytest.mark.parametrize("call", F.CALLS)
def test_the_family_reference_is_the_per_call_reference(call):
  c = SMALL[call]
  t = F.materialize(c)
  (o, lse, pmax, p2sum), vstat, storage = F.reference(c, t)
  T, hq = sum(c["qlens"]), c["heads"][0]
  assert o.shape == (T, 1, hq, F.DV) and lse.shape == pmax.shape == p2sum.shape == (T, hq, 1)
  want_o, want_lse = _per_call_reference(c, t, storage)
  assert torch.isfinite(o).all() and torch.allclose(o[:, 0], want_o, atol=1e-12, rtol=1e-12), (o[:, 0] - want_o).abs().max()
  assert torch.equal(torch.isneginf(lse[:, :, 0]), torch.isneginf(want_lse))
  fin = torch.isfinite(want_lse)
  assert torch.allclose(lse[:, :, 0][fin], want_lse[fin], atol=1e-12, rtol=1e-12)
  assert (o[:, 0][~fin] == 0).all() and (pmax[:, :, 0][~fin] == 0).all() and ((pmax > 0) & (pmax <= 1) | ~fin[:, :, None]).all()
  assert vstat[0] >= vstat[1] > 0


def _unused_is_nan(c, t, storage, live):
  """Every row of the view outside ``live`` (bool over the view's leading dims), and everything of the storage outside the view, holds NaN / 0xFF."""
  nan = (lambda x: x == 0xFF) if storage.dtype == torch.uint8 else torch.isnan
  view = R.reviewed(t["view"], t["storage"], storage)
  assert nan(view[~live]).all()
  outside = torch.ones_like(storage, dtype=torch.bool)
  R.reviewed(t["view"], t["storage"], outside).fill_(False)
  assert nan(storage[outside]).all() and int(outside.sum()) > 0


@pytest.mark.parametrize("call", F.CALLS)
def test_a_case_materializes_on_the_cpu_and_appends_where_the_contract_says(call):
  """Unused pages, rows behind a length, guard rows and padding hold NaN before the call; after it, row i of sequence b sits at ``max(len_b, 0) + i`` in the
  pool's format — rows at or past the capacity dropped — and nothing else of the storage has changed."""
  c = SMALL[call]
  t = F.materialize(c)
  _, _, after = F.reference(c, t)
  view, view_after = t["view"], R.reviewed(t["view"], t["storage"], after)
  live = torch.zeros(view.shape[:-2], dtype=torch.bool)
  want = t["storage"].clone()
  wview = R.reviewed(view, t["storage"], want)
  if c["sparse"]:
    flat_live, wflat = live.view(-1), (wview.flatten(0, 1) if wview.dim() == 4 else wview)
    stored = set(s for s in c.get("store_slots", ()) if 0 <= s < c["num_rows"])
    for row, n in zip(c["indices"], F.counts_of(c)):
      for s in row[:n]:
        flat_live[s] = s not in stored
    _unused_is_nan(c, t, t["storage"], live)
    for i, s in enumerate(c.get("store_slots", ())):
      if 0 <= s < c["num_rows"]:
        wflat[s] = F.encode(c, t["store_kv"][i])
    assert c["append"] == "none" or not torch.equal(want, t["storage"])
  else:
    page, cap, n_pages = view.size(1), c["capacity"], view.size(0)
    where = lambda b, p: (b if t["table"] is None else min(max(int(t["table"][b, p // page]), 0), n_pages - 1), p % page)
    for b, n in enumerate(c["lens"]):
      for p in range(min(max(n, 0), cap)):
        live[where(b, p)] = True
    _unused_is_nan(c, t, t["storage"], live)
    start, landed = 0, 0
    for b, n in enumerate(c["lens"]):
      for i in range(c["snew"][b] or 0):
        p = max(n, 0) + i
        if p < cap:
          wview[where(b, p)] = F.encode(c, (t["kv"][start + i] if c["ragged"] else t["kv"][b, i]))
          landed += 1
      start += c["qlens"][b] if c["ragged"] else 0
    assert landed > 0
  bits = lambda x: x.view(torch.int16) if x.element_size() == 2 else x
  assert torch.equal(bits(after), bits(want))
  assert view_after.shape == view.shape


def test_model_like_cases_show_their_family_property():
  """One seed in four lays a tests/model_values.py family out as latent rows; what the family promises is asserted on the rows the call computes on and on the
  family reference (the dequantised rows, for the quantised pools)."""
  model = [c for c in CASES if c["model"]]
  assert len({c["model"] for c in model}) >= 6 and {c["call"] for c in model} == set(F.CALLS)
  for c in model:
    t = F.materialize(c)
    us, _ = F.units(c, t)
    ref, _ = F.attend_units(us, c["scale"])
    assert all(u[1].size(0) in (389, 513) for u in us), c["seed"]
    F.assert_model_property(c, us, ref)


# ----------------------------------------------------------------------------- the checker bites
def _broken_units(n, seed):
  """Three causal tokens of 16 heads over two latent heads of ``n`` 656-byte rows: the intact units and the ways such kernels break."""
  from ffpa_attn_amd.kvcache import pack_latent_rows_ds, unpack_latent_rows_ds

  g = torch.Generator().manual_seed(seed)
  q = torch.randn((3, 16, F.D), generator=g).bfloat16()
  packed = pack_latent_rows_ds(torch.randn((n, 2, F.D), generator=g).bfloat16())
  rows = unpack_latent_rows_ds(packed).double()
  vis = torch.arange(n)[None, :] <= torch.arange(3)[:, None] + (n - 3)
  dropped = vis.clone()
  dropped[:, 32:64] = False
  wrong = packed.clone()
  wrong[..., 516:520] = wrong[..., 512:516]  # the scale of columns 0 ... 127 applied to columns 128 ... 255
  return (q, rows, vis), {
    "one 32-key tile dropped": (q, rows, dropped),
    "one tile counted twice": (q, torch.cat((rows, rows[32:64])), torch.cat((vis, vis[:, 32:64]), dim=1)),
    "a wrong scale on a 128-column tile": (q, unpack_latent_rows_ds(wrong).double(), vis),
  }


@pytest.mark.parametrize("n", [100, 4000])
def test_checker_rejects_the_family_reference_broken_the_way_kernels_break(n):
  good, broken = _broken_units(n, seed=n)
  ref, vstat = F.attend_units([good], F.SCALE)
  out, lse = ref[0].bfloat16(), ref[1].float()
  assert R.check(out, lse, ref, v=vstat, dtype="bf16", name="intact") <= 1.0
  bad = {what: F.attend_units([u], F.SCALE)[0][:2] for what, u in broken.items()}
  swap = [1, 0] + list(range(2, 16))
  bad["one head's rows swapped with its neighbour's"] = (ref[0][:, :, swap], ref[1][:, swap])
  assert len(bad) == 4
  for what, (o, l) in bad.items():
    with pytest.raises(AssertionError, match="max err|LSE"):
      R.check(o.bfloat16(), l.float(), ref, v=vstat, dtype="bf16", name=what)
    with pytest.raises(AssertionError, match="max err"):  # ... by the output alone, too
      R.check(o.bfloat16(), None, ref, v=vstat, dtype="bf16", name=what)
