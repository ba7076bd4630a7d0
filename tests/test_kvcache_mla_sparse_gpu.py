"""``ffpa_attn_with_kvcache_mla_sparse`` on the GPU: the gather build of the MLA latent-cache kernel — every wave reads the ids of its eight keys of a tile and
points its LDS-DMA pieces at the rows they name — against float64 attention on a contiguous cache built per token from ``pool[indices[t, :n_t]]``
(tests/kvcache_mla_sparse_ref.py: ``kvcache_ref.attend``; outputs held to ``kvcache_ref.check``: the suite's allowance, exact zeros / -inf for empty rows, no NaN
anywhere; no new tolerance).  D = 576, head_dim_v = 512, scale 1 / sqrt(192), T <= 6 tokens, pools of <= 1024 rows that hold NaN in every row no token selects.
Tiles hold 32 keys: the counts 0, 1, 31, 32, 33, 64, 97, 300 are the empty row, one key, each side of a tile, odd and even tile counts and a partial last tile."""

import contextlib

import pytest
import torch

import kvcache_mla_sparse_ref as SR
import kvcache_ref as R
from test_fwd_gpu import hip  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

D, DV = 576, 512
SCALE = 192 ** -0.5
NAN = float("nan")
COUNTS = [0, 1, 31, 32, 33, 64, 97, 300]
HEADS = [(16, 1), (72, 1), (128, 1), (32, 2)]


@contextlib.contextmanager
def _launches(hip, flags=0):
  """Every sparse launch inside the block carries ``flags`` too, and its plan (``plan_out``) is appended to the list the block receives."""
  plans, real = [], hip.mla_sparse_forward

  def spy(*args, **kw):
    plan = {}
    kw["flags"] = kw.get("flags", 0) | flags
    kw["plan_out"] = plan
    out = real(*args, **kw)
    plans.append(plan)
    return out

  hip.mla_sparse_forward = spy
  try:
    yield plans
  finally:
    hip.mla_sparse_forward = real


_CASES: dict = {}


def _case(counts, hq, hkv, dtype, topk=300, rows=1024, seed=0, tail="minus_one"):
  """q, the flat pool (NaN in every row no token selects), random slots WITH duplicates, the counts and the float64 reference: made once per shape and shared
  (nothing writes to it).  ``tail``: what stands at and past a row's count — -1, or in-range ids of NaN rows; neither may be read."""
  key = (tuple(counts), hq, hkv, dtype, topk, rows, seed, tail)
  if key in _CASES:
    return _CASES[key]
  g = torch.Generator(device="cuda").manual_seed(2000 + seed)
  gc = torch.Generator().manual_seed(seed)
  tdt = R.TORCH_DTYPE[dtype]
  T = len(counts)
  q = torch.randn((T, hq, D), generator=g, device="cuda", dtype=tdt)
  pool = torch.randn((rows, hkv, D), generator=g, device="cuda", dtype=tdt)
  live = torch.randperm(rows, generator=gc)[: rows // 2]  # slots are drawn from half of the pool: the other half stays NaN
  idx = live[torch.randint(0, live.numel(), (T, topk), generator=gc)]
  seen = torch.zeros(rows, dtype=torch.bool)
  for t, n in enumerate(counts):
    if n >= 2:
      idx[t, n - 1] = idx[t, 0]  # a duplicate in every row that has room for one
    seen[idx[t, :n]] = True
  dead = (~seen).nonzero().flatten()
  for t, n in enumerate(counts):
    idx[t, n:] = -1 if tail == "minus_one" else dead[torch.randint(0, dead.numel(), (topk - n,), generator=gc)]
  pool[~seen.cuda()] = NAN
  t = dict(q=q, pool=pool, idx=idx.to(torch.int32).cuda(), lens=torch.tensor(counts, dtype=torch.int32, device="cuda"), counts=list(counts), dtype=dtype,
           heads=(hq, hkv), topk=topk)
  t["ref"] = SR.reference(q, pool, t["idx"], counts, SCALE, DV)
  t["vstat"] = SR.visible_values(pool, t["idx"], counts, DV)
  _CASES[key] = t
  return t


def _sparse(hip, t, *, num_splits=0, flags=0, q=None, pool=None, idx=None, lens="case"):
  from ffpa_attn_amd import ffpa_attn_with_kvcache_mla_sparse

  with _launches(hip, flags) as plans:
    out, lse = ffpa_attn_with_kvcache_mla_sparse(t["q"] if q is None else q, t["pool"] if pool is None else pool, DV, t["idx"] if idx is None else idx,
                                                 topk_lens=t["lens"] if isinstance(lens, str) else lens, softmax_scale=SCALE, num_splits=num_splits,
                                                 return_softmax_lse=True)
  assert len(plans) == 1 and plans[0]["kernel"].startswith(f"ffpa_fwd_m16_mla_sparse_kernel<{t['dtype']}, 576, dv=512"), plans
  return out, lse, plans[0]


def _check(hip, t, what, ref=None, vstat=None, **kw):
  out, lse, plan = _sparse(hip, t, **kw)
  name = f"{what}: {t['dtype']} heads {t['heads']} counts {t['counts']} -> {plan}"
  T, hq = len(t["counts"]), t["heads"][0]
  assert out.shape == (T, hq, DV) and lse.shape == (hq, T) and lse.dtype == torch.float32
  ratio = R.check(out[:, None], lse.t()[:, :, None], t["ref"] if ref is None else ref, v=t["vstat"] if vstat is None else vstat, dtype=t["dtype"], name=name)
  print(f"[mla sparse] {ratio:.3f} {name}")
  return out, lse, plan


# ----------------------------------------------------------------------------- 1. counts x heads x dtypes
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("hq, hkv", HEADS)
@pytest.mark.parametrize("tail", ["minus_one", "nan_rows"])
def test_counts_heads_and_dtypes(hip, dtype, hq, hkv, tail):
  """Six tokens per launch, their counts drawn from the eight (two launches cover them all), topk = 300, random slots with duplicates; what stands at and past a
  row's count — -1, or in-range ids of NaN rows — is not read: the output is finite and right.  16 heads fill a quarter of a chunk, 72 are 64 + 8 rows, 128 two
  full chunks, (32, 2) two latent heads."""
  group = hq // hkv
  for part, counts in enumerate((COUNTS[:6], COUNTS[2:])):
    t = _case(counts, hq, hkv, dtype, seed=hq + part, tail=tail)
    out, lse, plan = _check(hip, t, f"counts ({tail})")
    assert plan["block_rows"] == 64 and plan["block_keys"] == 32 and plan["row_tiles"] == -(-group // 64), plan
    assert plan["workgroups"] == len(counts) * hkv * plan["row_tiles"] * plan["splits"], plan
    assert ("chunked" in plan["kernel"]) == (group > 64), plan
    for i, n in enumerate(counts):
      if n == 0:
        assert (out[i] == 0).all() and torch.isneginf(lse[:, i]).all()
  # no counts: every row holds topk valid entries
  full = _case([300, 300, 300], hq, hkv, dtype, seed=hq + 7)
  _check(hip, full, "topk_lens=None", lens=None)
  # the build whose pieces carry the non-temporal hint (the plan takes it for lists larger than the Infinity Cache: forced here)
  _, _, plan = _check(hip, full, "NT build", flags=hip.FLAG_KV_STREAM)
  assert ", NT>" in plan["kernel"], plan
  # counts outside [0, topk] are clamped
  t = _case(COUNTS[:6], hq, hkv, dtype, seed=hq, tail=tail)
  wild = t["lens"].clone()
  wild[0], wild[1] = -5, 1
  t300 = _case([300, 300, 300], hq, hkv, dtype, seed=hq + 7)
  _check(hip, t300, "counts past topk", lens=torch.tensor([301, 2 ** 30, 300], dtype=torch.int32, device="cuda"))
  out, lse, _ = _sparse(hip, t, lens=wild)
  assert (out[0] == 0).all() and torch.isneginf(lse[:, 0]).all()


# ----------------------------------------------------------------------------- 2. KV ranges
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("hq, hkv", [(16, 1), (128, 1), (32, 2)])
def test_forced_kv_ranges_start_at_odd_tiles(hip, dtype, hq, hkv):
  """num_splits 2, 3 and 5 forced over rows of 1 ... 10 tiles: every token shares out ITS tiles, so ranges start at odd tiles (the image parity follows the tile
  index; the ids of a range's first two tiles are read in its prologue) and some ranges are empty.  Then the library's own count on the same rows."""
  t = _case([1, 33, 64, 97, 160, 300], hq, hkv, dtype, seed=50 + hq)
  for ns in (2, 3, 5):
    out, lse, plan = _check(hip, t, "KV ranges", num_splits=ns, flags=hip.FLAG_FORCE_SPLITS)
    assert plan["splits"] == ns and plan["kernel"].endswith("+ ffpa_varlen_merge_kernel"), plan
  out0, lse0, plan0 = _check(hip, t, "the library's own count")
  assert plan0["workgroups"] == 6 * hkv * plan0["row_tiles"] * plan0["splits"], plan0


# ----------------------------------------------------------------------------- 3. the same arithmetic as the dense latent call
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("ns", [1, 3])
@pytest.mark.parametrize("hq", [16, 128])
def test_same_arithmetic_as_the_dense_latent_call(hip, dtype, ns, hq):
  """indices[t] = the slots of sequence t's keys in order (a page-64 pool behind a shuffled block table): the sparse launch reads the same rows into the same LDS
  image, so at the same forced number of ranges the LSE is the same bits in both dtypes and O in bf16; fp16 O may differ by one ulp (the compiler's
  last-instruction rounding, the allowance the latent suite gives its own twin)."""
  from ffpa_attn_amd import ffpa_attn_with_kvcache_mla, slots_from_block_table

  lens_l = [1, 33, 64, 97, 300, 0]
  T, page, pps = len(lens_l), 64, 5
  g = torch.Generator(device="cuda").manual_seed(300 + hq)
  tdt = R.TORCH_DTYPE[dtype]
  q = torch.randn((T, hq, D), generator=g, device="cuda", dtype=tdt)
  n_pages = T * pps + 1
  pool = torch.randn((n_pages, page, 1, D), generator=g, device="cuda", dtype=tdt)
  table = torch.randperm(n_pages, generator=torch.Generator().manual_seed(3))[: T * pps].to(torch.int32).view(T, pps).cuda()
  lens = torch.tensor(lens_l, dtype=torch.int32, device="cuda")
  pos = torch.arange(pps * page, dtype=torch.int32, device="cuda").expand(T, -1)
  idx = slots_from_block_table(pos, table, page)
  flags = hip.FLAG_FORCE_SPLITS if ns > 1 else 0
  plan_d = {}
  real = hip.mla_forward
  hip.mla_forward = lambda *a, **kw: real(*a, **dict(kw, flags=kw.get("flags", 0) | flags, plan_out=plan_d))
  try:
    want, want_lse = ffpa_attn_with_kvcache_mla(q[:, None], pool, DV, cache_seqlens=lens, block_table=table, softmax_scale=SCALE, num_splits=ns, return_softmax_lse=True)
  finally:
    hip.mla_forward = real
  t = dict(q=q, pool=pool, idx=idx, lens=lens, dtype=dtype)
  out, lse, plan = _sparse(hip, t, num_splits=ns, flags=flags)
  assert plan["splits"] == plan_d["splits"] == ns and plan["row_tiles"] == plan_d["row_tiles"], (plan, plan_d)
  want, want_lse = want[:, 0], want_lse[:, :, 0].t()
  assert torch.equal(lse, want_lse)
  if dtype == "bf16":
    assert torch.equal(out, want), f"{int((out != want).sum())} elements differ, max {(out.float() - want.float()).abs().max().item():.3e}"
  else:
    assert ((out.double() - want.double()).abs() <= R.ulp_of(want.double(), dtype)).all()


# ----------------------------------------------------------------------------- 4. pool layouts
@pytest.mark.parametrize("layout", ["flat", "page1", "page16", "page64", "row_padded", "head_padded"])
def test_pool_layouts_and_strided_arguments(hip, layout):
  """The flat 3-D pool, 4-D pools of page size 1 / 16 / 64, a padded row stride and a padded head stride; q as a slice of a fused projection, indices as
  ``wide[:, 5:5 + topk]`` of a wider tensor (its other columns hold ids far outside the pool), topk_lens as ``buf[::2]``.  Everything a storage holds outside the
  pool's view is NaN."""
  hq, hkv = 32, 2
  t = _case([1, 33, 97, 300, 0, 64], hq, hkv, "bf16", seed=90)
  flat = t["pool"]
  rows = flat.size(0)
  if layout == "flat":
    pool = flat.clone()
  elif layout.startswith("page"):
    page = int(layout[4:])
    pool = flat.clone().view(rows // page, page, hkv, D)
  elif layout == "row_padded":
    store = torch.full((rows, hkv * D + 64), NAN, dtype=flat.dtype, device="cuda")
    pool = store[:, : hkv * D].view(rows, hkv, D)
    pool.copy_(flat)
  else:
    store = torch.full((rows, hkv, D + 64), NAN, dtype=flat.dtype, device="cuda")
    pool = store[..., :D]
    pool.copy_(flat)
  fused = torch.full((6, hq + 2, D), NAN, dtype=flat.dtype, device="cuda")
  fused[:, :hq] = t["q"]
  wide = torch.full((6, t["topk"] + 9), 2 ** 30, dtype=torch.int32, device="cuda")
  wide[:, 5:5 + t["topk"]] = t["idx"]
  buf = torch.full((12,), 2 ** 30, dtype=torch.int32, device="cuda")
  buf[::2] = t["lens"]
  out, lse, plan = _check(hip, t, f"layout {layout}", q=fused[:, :hq], pool=pool, idx=wide[:, 5:5 + t["topk"]], lens=buf[::2])
  plain = _sparse(hip, t)
  assert torch.equal(out, plain[0]) and torch.equal(lse, plain[1])  # (the same rows through other strides: the same bits)


# ----------------------------------------------------------------------------- 5. one graph
def test_one_graph_follows_the_step_s_tensors_written_in_place(hip):
  """Captured once — a split launch: the merge is in the graph —, then q, indices, topk_lens and pool rows are overwritten in place: every replay equals a fresh
  eager call bit for bit (and the float64 reference)."""
  from ffpa_attn_amd import ffpa_attn_with_kvcache_mla_sparse

  t = _case([5, 300, 64, 97], 16, 1, "bf16", seed=120)
  pool = t["pool"].clone().nan_to_num_(nan=0.25)  # (replays move the lists around: every row must hold a number)
  q, idx, lens = t["q"].clone(), t["idx"].clone(), t["lens"].clone()
  idx.clamp_(min=0)
  call = lambda: ffpa_attn_with_kvcache_mla_sparse(q, pool, DV, idx, topk_lens=lens, softmax_scale=SCALE, num_splits=3, return_softmax_lse=True)
  with _launches(hip, hip.FLAG_FORCE_SPLITS) as plans:  # (three ranges, forced: in the warm call, in the capture and in the eager calls alike)
    call()  # (warm: the library is loaded, the scratch is sized)
    assert plans[0]["splits"] == 3 and plans[0]["kernel"].endswith("+ ffpa_varlen_merge_kernel"), plans
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
      out_g, lse_g = call()
    gc = torch.Generator().manual_seed(5)
    for step, counts in enumerate(([5, 300, 64, 97], [0, 33, 300, 1], [300, 31, 32, 160])):
      if step:
        q.copy_(torch.randn_like(q))
        idx.copy_(torch.randint(0, pool.size(0), tuple(idx.shape), generator=gc).to(torch.int32))
        rows = torch.randperm(pool.size(0), generator=gc)[:100].cuda()
        pool[rows] = torch.randn((100, 1, D), device="cuda").to(pool.dtype)
      lens.copy_(torch.tensor(counts, dtype=torch.int32, device="cuda"))
      graph.replay()
      torch.cuda.synchronize()
      eager = call()
      torch.cuda.synchronize()
      assert torch.equal(out_g, eager[0]) and torch.equal(lse_g, eager[1]), counts
      R.check(out_g[:, None], lse_g.t()[:, :, None], SR.reference(q, pool, idx, counts, SCALE, DV), v=SR.visible_values(pool, idx, counts, DV), dtype="bf16",
              name=f"graph replay at {counts}")


# ----------------------------------------------------------------------------- 6. torch.compile
def test_under_torch_compile_fullgraph(hip):
  from ffpa_attn_amd import compact_topk_indices, ffpa_attn_with_kvcache_mla_sparse

  t = _case([33, 0, 97, 300], 16, 1, "fp16", seed=130)

  def f(q, pool, idx):
    slots, counts = compact_topk_indices(idx)  # (rows padded with -1 behind their count: already compact, counted here)
    o, lse = ffpa_attn_with_kvcache_mla_sparse(q, pool, DV, slots, topk_lens=counts, softmax_scale=SCALE, return_softmax_lse=True)
    return o * 2, lse

  eager = f(t["q"], t["pool"], t["idx"])
  compiled = torch.compile(f, fullgraph=True)(t["q"], t["pool"], t["idx"])
  torch.cuda.synchronize()
  assert torch.equal(eager[0], compiled[0]) and torch.equal(eager[1], compiled[1])
  R.check((compiled[0].double() / 2).to(torch.float16)[:, None], compiled[1].t()[:, :, None], t["ref"], v=t["vstat"], dtype="fp16", name="torch.compile")


# ----------------------------------------------------------------------------- 7. permutation
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_a_permuted_index_row_stays_inside_the_allowance(hip, dtype):
  """The keys of a row in another order are the same attention: the result stays inside the allowance of the SAME float64 reference (it is not the same bits —
  the running max and the fp32 sums meet the keys in another order — and nothing here asks for that)."""
  t = _case([33, 97, 300, 64], 16, 1, dtype, seed=140)
  idx = t["idx"].clone()
  gc = torch.Generator().manual_seed(9)
  for i, n in enumerate(t["counts"]):
    idx[i, :n] = idx[i, :n][torch.randperm(n, generator=gc).cuda()]
  _check(hip, t, "permuted rows", idx=idx)


# ----------------------------------------------------------------------------- the contract on bad entries
def test_entries_outside_the_pool_in_front_of_the_count_are_clamped_not_followed(hip):
  """An entry in front of the count that lies outside [0, num_rows) is clamped into the pool: the call stays memory-safe; that token's result is unspecified,
  every other token's is right."""
  t = _case([33, 97, 300, 64], 16, 1, "bf16", seed=150)
  idx = t["idx"].clone()
  idx[1, 5], idx[1, 40] = 2 ** 31 - 1, -(2 ** 31)
  out, lse, _ = _sparse(hip, t, idx=idx)
  torch.cuda.synchronize()
  keep = [0, 2, 3]
  ref = tuple(x[keep] for x in t["ref"])
  R.check(out[keep][:, None], lse.t()[keep][:, :, None], ref, v=t["vstat"], dtype="bf16", name="tokens next to a bad row")
