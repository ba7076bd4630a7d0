"""The float64 KV-cache reference (tests/kvcache_ref.py) and its checker, shown to bite without a GPU: the reference against SDPA / complex multiplication / plain
indexing, the checker against outputs broken the way such kernels break (at 100 keys and at 16k), and the sweep's generator against its coverage conditions."""

import collections

import pytest
import torch
import torch.nn.functional as F

import kvcache_ref as R


def _pool_case(n, dtype, seed=0, page=64, hq=4, hkv=2, d=64, sq=2, snew=2, B=2):
  """A paged cache of B sequences of ``n`` and ``n - 7`` ... keys (before the append), shuffled pages, + new keys, rotary tables and q."""
  g = torch.Generator().manual_seed(seed)
  pps = -(-(n + snew) // page) + 1
  n_pages = B * pps + 2
  table = torch.randperm(n_pages, generator=g)[:B * pps].to(torch.int32).view(B, pps)
  rnd = lambda *s: torch.randn(s, generator=g).to(dtype)
  ang = torch.rand((pps * page, d // 2), generator=g, dtype=torch.float64) * 6.283185307179586
  return {"kc": rnd(n_pages, page, hkv, d), "vc": rnd(n_pages, page, hkv, d), "table": table, "lens": [n - snew - 7 * b for b in range(B)], "q": rnd(B, sq, hq, d),
          "k": rnd(B, snew, hkv, d), "v": rnd(B, snew, hkv, d), "cos": torch.cos(ang).to(dtype), "sin": torch.sin(ang).to(dtype)}


def _run(c, dtype, *, table=None, lens_cut=0, cos_shift=0, interleaved=True, diagonal=0, kc_of=None, vc_of=None):
  """The call on a case, with the breakages of the mutation test as options -> attend's tuple."""
  kc, vc = c["kc"].clone(), c["vc"].clone()
  cos, sin = c["cos"][cos_shift:], c["sin"][cos_shift:]
  q_rot, used, _ = R.append(kc, vc, c["k"], c["v"], c["lens"], c["table"], cos, sin, interleaved, True, q=c["q"])
  q = q_rot.to(dtype)
  used = [u - lens_cut for u in used]
  if diagonal:  # the causal diagonal one key lower: the rows of a call of Sq + 1 tokens
    q = torch.cat((q, q[:, -1:]), dim=1)
  ref = R.attend(q, kc if kc_of is None else kc_of(kc, vc), vc if vc_of is None else vc_of(kc, vc), used, c["table"] if table is None else table, True)
  if diagonal:
    ref = (ref[0][:, :-1], ref[1][..., :-1], ref[2][..., :-1], ref[3][..., :-1])
  return ref, (kc, vc, used)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("n", [100, 16384])
def test_checker_rejects_every_broken_output_and_accepts_the_true_one(n, dtype):
  """The reference's own output rounded to 16 bits stands in for the kernel's; then one thing is broken at a time.  The checker must reject each — at 16k keys,
  where one wrong page or tile is 0.4 % of a row, as well as at 100 — and accept the unbroken one."""
  c = _pool_case(n, dtype, seed=n)
  ref, (kc, vc, used) = _run(c, dtype)
  vstat = R.visible_values(vc, used, c["table"])
  good = ref[0].to(dtype)
  ratio = R.check(good, ref[1].float(), ref, v=vstat, dtype=dtype, name="intact")
  assert ratio <= 1.0
  other = c["table"].clone()
  other[0, (n // 64) // 2] = c["table"][1, 0]  # one page of sequence 0 is another sequence's
  broken = {
    "a page swapped for another": dict(table=other),
    "the last 64-key tile dropped": dict(lens_cut=64),
    "the rotary position off by one": dict(cos_shift=1),
    "interleaved taken for NeoX": dict(interleaved=False),
    "the causal diagonal shifted by one": dict(diagonal=1),
    "a KV head's group mapped to the neighbouring head": dict(kc_of=lambda k, v: k.flip(2), vc_of=lambda k, v: v.flip(2)),
    "the K half read where the V half belongs": dict(vc_of=lambda k, v: k),
  }
  for what, how in broken.items():
    bad = _run(c, dtype, **how)[0]
    with pytest.raises(AssertionError, match="max err|LSE"):
      R.check(bad[0].to(dtype), bad[1].float(), ref, v=vstat, dtype=dtype, name=what)
    with pytest.raises(AssertionError, match="max err"):  # ... by the output alone, too
      R.check(bad[0].to(dtype), None, ref, v=vstat, dtype=dtype, name=what)


def test_cache_checker_rejects_a_write_into_the_neighbouring_half():
  """check_cache: a rotated row off by two ulps, one V element written into the K half next to it, one padding element touched — each rejected."""
  dtype = torch.bfloat16
  c = _pool_case(200, dtype, seed=3)
  kview, vview, ks, vs = R.lay_out_cache(c["kc"], c["vc"], "kv_dim1", fill=0.5)
  want = ks.clone()
  wk, wv = R.reviewed(kview, ks, want), R.reviewed(vview, vs, want)
  _, _, rotated = R.append(wk, wv, c["k"], c["v"], c["lens"], c["table"], c["cos"], c["sin"], True, True)
  R.check_cache(want.clone(), want, R.reviewed(kview, ks, want.clone()), wk, rotated, 64, "intact")
  page, row = rotated[0]
  for what, where in (("rotated", (page, 0, row, 0, 3)), ("v half", (page, 1, row, 1, 5)), ("other page", ((page + 1) % want.size(0), 0, 1, 0, 0))):
    got = want.clone()
    got[where] = got[where] * (1 + 2.0 ** -6) + 2.0 ** -9
    with pytest.raises(AssertionError):
      R.check_cache(got, want, R.reviewed(kview, ks, got), wk, rotated, 64, what)


@pytest.mark.parametrize("causal", [False, True])
def test_attend_is_sdpa_in_float64(causal):
  """Small ragged batches, GQA, rows without a key (length 0; more tokens than keys under causal), a contiguous and a paged cache."""
  g = torch.Generator().manual_seed(1)
  B, sq, hq, hkv, d, cap = 4, 5, 6, 2, 24, 40
  lens = [0, 3, 17, 40]
  q = torch.randn((B, sq, hq, d), generator=g, dtype=torch.float64)
  kc, vc = torch.randn((B, cap, hkv, d), generator=g, dtype=torch.float64), torch.randn((B, cap, hkv, d), generator=g, dtype=torch.float64)
  pool_k, pool_v = kc.reshape(B * 5, 8, hkv, d), vc.reshape(B * 5, 8, hkv, d)  # the same keys as pages of 8
  table = torch.arange(B * 5, dtype=torch.int32).view(B, 5)
  for k_, v_, tbl in ((kc, vc, None), (pool_k, pool_v, table)):
    o, lse, pmax, p2sum = R.attend(q, k_, v_, lens, tbl, causal)
    for b, n in enumerate(lens):
      i, j = torch.arange(sq)[:, None], torch.arange(n)[None, :]
      mask = (j <= i + n - sq) if causal else torch.ones((sq, n), dtype=torch.bool)
      live = mask.any(dim=1)
      kb, vb = (t[b, :n].transpose(0, 1).repeat_interleave(hq // hkv, 0) for t in (kc, vc))
      s = torch.einsum("shd,hnd->hsn", q[b], kb) * d ** -0.5
      s = s.masked_fill(~mask[None], float("-inf"))
      if n:
        want = F.scaled_dot_product_attention(q[b].transpose(0, 1)[None], kb[None], vb[None], attn_mask=mask[None, None])[0].transpose(0, 1)
        assert torch.allclose(o[b][live], want[live], atol=1e-12, rtol=1e-12)
        p = torch.softmax(s[:, live], dim=-1)
        assert torch.allclose(pmax[b][:, live], p.amax(-1), atol=1e-14) and torch.allclose(p2sum[b][:, live], p.pow(2).sum(-1), atol=1e-14)
        assert torch.allclose(lse[b][:, live], torch.logsumexp(s[:, live], dim=-1), atol=1e-12)
      assert (o[b][~live] == 0).all() and torch.isneginf(lse[b][:, ~live]).all()


@pytest.mark.parametrize("interleaved", [True, False])
def test_rotation_is_complex_multiplication(interleaved):
  g = torch.Generator().manual_seed(2)
  s, h, d, rd, ro = 5, 3, 40, 16, 9
  x = torch.randn((s, h, d), generator=g, dtype=torch.float64)
  ang = torch.rand((ro, rd // 2), generator=g, dtype=torch.float64) * 6.0
  pos = [2, 3, 8, 9, 30]  # (9 and 30 clamp to seqlen_ro - 1 = 8)
  got = R.rotate(x, torch.cos(ang), torch.sin(ang), pos, interleaved)
  a, b = (x[..., 0:rd:2], x[..., 1:rd:2]) if interleaved else (x[..., :rd // 2], x[..., rd // 2:rd])
  z = torch.complex(a, b) * torch.polar(torch.ones_like(ang), ang)[[min(p, ro - 1) for p in pos]][:, None, :]
  want = x.clone()
  if interleaved:
    want[..., 0:rd:2], want[..., 1:rd:2] = z.real, z.imag
  else:
    want[..., :rd // 2], want[..., rd // 2:rd] = z.real, z.imag
  assert torch.allclose(got, want, atol=1e-14) and torch.equal(got[..., rd:], x[..., rd:])


@pytest.mark.parametrize("layout", R.POOL_LAYOUTS)
def test_gather_and_append_are_plain_indexing_on_any_view(layout):
  """Shared pages, ids below 0 and past the pool (the documented clamp), every strided layout; the append lands where plain indexing says, straddles a page
  boundary and the capacity, and leaves every other element of the storage alone."""
  g = torch.Generator().manual_seed(4)
  n_pages, page, h, d = 6, 4, 2, 8
  kc, vc = torch.randn((n_pages, page, h, d), generator=g).bfloat16(), torch.randn((n_pages, page, h, d), generator=g).bfloat16()
  kview, vview, ks, vs = R.lay_out_cache(kc, vc, layout, fill=7.0)
  assert torch.equal(kview, kc) and torch.equal(vview, vc)
  table = R.lay_out_table(torch.tensor([[3, 1, -5], [3, 99, 0]], dtype=torch.int32), "wide_slice")  # page 3 shared; -5 -> 0, 99 -> 5
  for b, n in ((0, 11), (1, 12)):
    gk, gv = R.gather(kview, vview, table, b, n)
    for j in range(n):
      pid = min(max(int(table[b, j // page]), 0), n_pages - 1)
      assert torch.equal(gk[j], kc[pid, j % page]) and torch.equal(gv[j], vc[pid, j % page])
  before_k, before_v = ks.clone(), vs.clone()
  newk, newv = torch.randn((2, 3, h, d), generator=g).bfloat16(), torch.randn((2, 3, h, d), generator=g).bfloat16()
  _, used, _ = R.append(kview, vview, newk, newv, [3, 10], table)  # sequence 0: rows 3, 4, 5 (pages 3 -> 1); sequence 1: rows 10, 11, then the capacity (12)
  assert used == [6, 12]
  want_k, want_v = kc.clone(), vc.clone()
  for (pid, row), (b, i) in {(3, 3): (0, 0), (1, 0): (0, 1), (1, 1): (0, 2), (0, 2): (1, 0), (0, 3): (1, 1)}.items():
    want_k[pid, row], want_v[pid, row] = newk[b, i], newv[b, i]
  assert torch.equal(kview, want_k) and torch.equal(vview, want_v)
  for view, storage, before in ((kview, ks, before_k), (vview, vs, before_v)):  # nothing but the views' own elements moved
    outside = torch.ones_like(storage, dtype=torch.bool)
    R.reviewed(view, storage, outside).fill_(False)
    if ks is vs:
      R.reviewed(vview if view is kview else kview, storage, outside).fill_(False)
    assert torch.equal(storage[outside], before[outside])
  slab_k, slab_v = kc.clone(), vc.clone()  # the same tensors as a contiguous cache of 6 slabs of 4 keys
  assert torch.equal(R.gather(slab_k, slab_v, None, 4, 3)[0], kc[4, :3])


def test_sweep_generator_covers_its_axes():
  """Asserted from the generator alone, over the committed seeds: every axis value at least 5 times; at least 80 % of all query rows see a key and at most 10 %
  of the cases see none at all; every head-dim class the paged kernel is built for with both dtypes (in a PAGED case)."""
  cases = [R.draw_case(s) for s in R.SWEEP_SEEDS]
  axes = {"entry": R.ENTRIES, "layout": R.POOL_LAYOUTS, "page": R.PAGES, "dtype": ("bf16", "fp16"), "heads": R.HEADS, "B": range(1, 10), "num_splits": R.SPLITS,
          "stream": R.STREAMS, "causal": (False, True), "return_lse": (False, True), "lens_strided": (False, True), "fused_qkv": (False, True),
          "interleaved": (False, True)}
  for axis, values in axes.items():
    count = collections.Counter(c[axis] for c in cases)
    for value in values:
      assert count[value] >= 5, (axis, value, count)
  paged = [c for c in cases if c["page"]]
  tl = collections.Counter(c["table_layout"] for c in paged)
  assert all(tl[v] >= 5 for v in R.TABLE_LAYOUTS), tl
  sq = collections.Counter(c["Sq"] for c in cases)
  assert all(sq[v] >= 5 for v in range(1, 7)) and sum(n for v, n in sq.items() if 65 <= v <= 300) >= 5, sq
  assert sum(1 for c in cases if c["rotary_dim"]) >= 5 and sum(1 for c in cases if c["Snew"] == 0) >= 1
  assert {(c["head_dim_class"], c["dtype"]) for c in paged} == {(d, t) for d in R.PAGED_HEAD_DIM_CLASSES for t in ("bf16", "fp16")}
  assert sum(1 for c in cases if c["D"] != c["head_dim_class"]) >= 5  # head dims between the built ones
  for c in cases:
    assert c["D"] % 8 == 0 and 8 <= c["D"] <= 1024 and (c["D"] + 63) // 64 * 64 == max(c["head_dim_class"], 64) or c["D"] < 128, c
  seen, rows = (sum(x) for x in zip(*(R.visible_rows(c) for c in cases)))
  assert seen >= 0.8 * rows, (seen, rows)
  assert sum(1 for c in cases if R.visible_rows(c)[0] == 0) <= 0.1 * len(cases)
  edge = collections.Counter()
  for c in cases:
    unit = c["page"] or 64
    for n in c["lens"]:
      for name, hit in (("zero", n == 0), ("negative", n < 0), ("capacity", n == c["capacity"]), ("above", n > c["capacity"]), ("page + 1", n == unit + 1), ("page - 1", n == unit - 1)):
        edge[name] += hit
  assert all(edge[name] >= 1 for name in ("zero", "negative", "capacity", "above", "page + 1", "page - 1")), edge
  assert sum(c["bad_unused_ids"] for c in cases) >= 5 and sum(c["bad_used_id"] for c in cases) >= 1 and sum(c["share_prefix_pages"] for c in cases) >= 1


def test_a_drawn_case_materializes_on_the_cpu_and_its_reference_runs():
  """Drawing and building a case needs no GPU; the reference's post-append storage differs from the original in the appended rows only."""
  for seed in (2, 5, 11):
    c = R.draw_case(seed)
    t = R.materialize(c)
    ref, kview, vview, ks, vs, rotated = R.reference(c, t)
    assert ref[0].shape == t["q"].shape and ref[1].shape == (c["B"], c["heads"][0], c["Sq"])
    changed = (ks.view(torch.int16) != t["k_storage"].view(torch.int16)).sum().item()
    if c["Snew"] is not None:
      hkv = c["heads"][1]
      landed = sum(max(0, min(max(n, 0) + c["Snew"], c["capacity"]) - min(max(n, 0), c["capacity"])) for n in c["lens"])
      assert 0 < changed <= landed * hkv * c["D"] * (2 if ks is vs else 1)
    else:
      assert changed == 0
