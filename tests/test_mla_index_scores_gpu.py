"""``ffpa_mla_index_scores`` on the GPU against its definition in float64 on the very 16-bit inputs: the WHOLE ``[T, N]`` tensor, -inf columns exactly -inf, a finite
column within ``(128 + Hi + 8) * 2^-23 * A[t, p]``, ``A = sum_h |w| sum_d |q k|`` in float64 — the worst case of fp32 accumulation in any order with chopped or
rounded partial sums (128 products and Hi weighted terms, the relu 1-Lipschitz), derived, not measured.  Then exact integer inputs end to end into the selection,
and the three launches scores -> selection -> sparse attention in one HIP graph."""

import pytest
import torch

import kvcache_mla_sparse_topk_ref as TR
from ffpa_attn_amd.hip import MLA_INDEX_CHUNK_KEYS as C
from test_fwd_gpu import hip  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

NINF = float("-inf")
LENGTHS = [1, 63, 64, 65, C - 1, C + 1, 2 * C + 17]  # the lengths at which the kernel can go wrong: a step, a wave's quarter, a chunk
DTYPES = [torch.bfloat16, torch.float16]


def _i32(x):
  return torch.tensor(x, dtype=torch.int32, device="cuda")


def reference(q, k, w, lens, table, N, cu=None, causal=True):
  """The definition in float64 on CPU copies -> ``(scores [T, N], A [T, N])``."""
  q, k, w, lens = q.cpu().double(), k.cpu().double().reshape(k.size(0), k.size(1), 128), w.cpu().double(), lens.cpu()
  T, ps, W = q.size(0), k.size(1), 1 if table is None else table.size(1)
  out, A = torch.full((T, N), NINF, dtype=torch.float64), torch.zeros((T, N), dtype=torch.float64)
  for t, where in enumerate(TR.token_sequences(T, lens, None if cu is None else cu.cpu())):
    if where is not None:
      b, i, S = where
      p = torch.arange(min(TR.visible(int(lens[b]), S, i, N, causal), W * ps))
      page = torch.full_like(p, b) if table is None else table[b].cpu().long()[(p // ps).clamp(max=W - 1)].clamp(0, k.size(0) - 1)
      keys = k[page, p % ps]
      out[t, :p.numel()] = (w[t, :, None] * (q[t] @ keys.T).clamp(min=0)).sum(0)
      A[t, :p.numel()] = (w[t, :, None].abs() * (q[t].abs() @ keys.abs().T)).sum(0)
  return out, A


def check(got, want, A, Hi, what=""):
  got = got.cpu()
  assert got.dtype == torch.float32 and got.shape == want.shape and got.is_contiguous()
  tail = want == NINF
  assert torch.equal(got == NINF, tail), f"{what}: the -inf columns differ in {int(((got == NINF) != tail).sum())} places"
  err, bound = (got.double() - want)[~tail].abs(), (128 + Hi + 8) * 2.0 ** -23 * A[~tail]
  print(f"{what}: max err / bound = {float((err / bound.clamp(min=1e-300)).max()) if err.numel() else 0.0:.4f}")
  assert bool((err <= bound).all()), f"{what}: {int((err > bound).sum())} columns past the bound, worst {float((err - bound).max())}"


def inputs(T, Hi, dtype, seed, strided=False, ints=False):
  """q ~ N(0, 1) in the dtype and weights of mixed signs (cancellation) — or integers in [-3, 3] and +-{1/4, 1/2, 1, 2}; ``strided``: views with a storage offset."""
  g = torch.Generator(device="cuda").manual_seed(seed)
  shape_q, shape_w = ((T + 1, Hi + 1, 136), (T + 1, Hi + 3)) if strided else ((T, Hi, 128), (T, Hi))
  if ints:
    q = torch.randint(-3, 4, shape_q, generator=g, device="cuda").to(dtype)
    w = (2.0 ** torch.randint(-2, 2, shape_w, generator=g, device="cuda")) * (2 * torch.randint(0, 2, shape_w, generator=g, device="cuda") - 1)
  else:
    q, w = torch.randn(shape_q, generator=g, device="cuda").to(dtype), torch.randn(shape_w, generator=g, device="cuda") * Hi ** -0.5
  return (q[1:, 1:, 8:], w[1:, 3:]) if strided else (q, w.float())


def cache(layout, lens, dtype, seed, ints=False, spare=2):
  """-> ``(k_index_cache, block_table | None)`` for sequences of ``lens`` keys.  Paged: a shuffled pool; behind every sequence's last used page the table holds
  ids far outside the pool (never read)."""
  g = torch.Generator(device="cuda").manual_seed(seed)
  make = (lambda s: torch.randint(-3, 4, s, generator=g, device="cuda").to(dtype)) if ints else (lambda s: torch.randn(s, generator=g, device="cuda").to(dtype))
  B = len(lens)
  if layout == "contiguous":
    return make((B, -(-max(max(lens), 1) // 64) * 64, 128)), None
  page = int(layout)
  used = [-(-max(L, 0) // page) for L in lens]
  W, pages = max(used) + spare, sum(used) + 3
  ids = torch.randperm(pages, generator=torch.Generator().manual_seed(seed)).tolist()
  table = torch.tensor([2 ** 31 - 1, -(2 ** 31)] * B * W)[:B * W].view(B, W).clone()
  for b in range(B):
    table[b, :used[b]] = torch.tensor(ids[sum(used[:b]):sum(used[:b + 1])], dtype=torch.int64)
  k = make((pages, page, 1, 128) if page == 64 else (pages, page, 128))
  return k, table.to(torch.int32).cuda()


# ----------------------------------------------------------------------------- 1. against float64
@pytest.mark.parametrize("layout", ["64", "128", "contiguous"])
@pytest.mark.parametrize("Hi", [32, 64])
@pytest.mark.parametrize("dtype", DTYPES)
def test_every_length_against_float64(dtype, Hi, layout):
  """One token per sequence, one sequence per length of LENGTHS, N past the longest: the tail of every row is -inf."""
  from ffpa_attn_amd import ffpa_mla_index_scores

  N = max(LENGTHS) + 30
  q, w = inputs(len(LENGTHS), Hi, dtype, 1)
  k, table = cache(layout, LENGTHS, dtype, 2)
  got = ffpa_mla_index_scores(q, k, w, _i32(LENGTHS), table, max_seqlen_k=N)
  want, A = reference(q, k, w, _i32(LENGTHS), table, N)
  assert [int((r != NINF).sum()) for r in want] == LENGTHS
  check(got, want, A, Hi, f"{dtype} Hi {Hi} {layout}")


@pytest.mark.parametrize("case", ["causal3", "noncausal3", "clamp", "ragged", "table_inside", "table_short"])
@pytest.mark.parametrize("dtype, Hi, layout", [(torch.bfloat16, 64, "64"), (torch.float16, 32, "128"), (torch.bfloat16, 32, "contiguous")])
def test_token_rules_against_float64(dtype, Hi, layout, case):
  """Sq = 3 causal (tokens whose n_t is <= 0 included) and non-causal; N below the lengths; a ragged step with an empty sequence, padding rows and strided
  q_index / weights; a page id outside the pool INSIDE a sequence (clamped, as the reference clamps it); a table too narrow for the lengths."""
  from ffpa_attn_amd import ffpa_mla_index_scores

  lens_l, cu, causal, N = [1, 2, 65, C + 1, 2 * C + 17, 0], None, True, 2 * C + 80
  T = 3 * len(lens_l)
  if case == "noncausal3":
    causal = False
  elif case == "clamp":
    N = C - 3
  elif case == "ragged":
    cu, T = _i32([0, 2, 2, 7, 8, 9, 9]), 12  # (sequence 1 and 5 have no token; rows 9 ... 11 are padding)
  q, w = inputs(T, Hi, dtype, 3, strided=case == "ragged")
  k, table = cache(layout, lens_l, dtype, 4, spare=0 if case == "table_short" else 2)
  lens = _i32(lens_l)
  if case == "table_inside" and table is not None:
    table[4, 1], table[3, 0] = 10 ** 9, -5
  if case == "table_short":
    lens = lens + 300  # (lengths past what the table / the capacity can name: n_t stops there)
  got = ffpa_mla_index_scores(q, k, w, lens, table, max_seqlen_k=N, cu_seqlens_q=cu, causal=causal)
  want, A = reference(q, k, w, lens, table, N, cu, causal)
  if case == "causal3":
    assert bool((want[0] == NINF).all()) and bool((want[2, :1] != NINF).all())  # (token 0 of 3 of a sequence of length 1 sees nothing)
  check(got, want, A, Hi, f"{case} {dtype} Hi {Hi} {layout}")


def test_a_first_element_off_16_bytes_is_the_c_layers_refusal():
  """The Python checks read no ``data_ptr`` (they trace under ``torch.compile``): the C status speaks, before any device work."""
  from ffpa_attn_amd import ffpa_mla_index_scores

  q, w = inputs(2, 32, torch.bfloat16, 1)
  k = torch.zeros((2, 64, 136), dtype=torch.bfloat16, device="cuda")[:, :, 4:132]
  with pytest.raises(ValueError, match="16-byte aligned"):
    ffpa_mla_index_scores(q, k, w, _i32([5, 5]), max_seqlen_k=64)


# ----------------------------------------------------------------------------- 2. exact, and end to end
@pytest.mark.parametrize("dtype", DTYPES)
def test_integer_inputs_are_exact_and_feed_the_selection(dtype):
  """q, k integers in [-3, 3], weights +-{1/4, 1/2, 1, 2}: every fp32 operation is exact, whatever its order — the scores EQUAL the float64 definition, and the
  selection over them (many ties: the stable rule) equals the definition's over the reference scores."""
  from ffpa_attn_amd import ffpa_mla_index_scores, ffpa_mla_sparse_topk_slots

  Hi, L, page, topk = 64, 2 * C + 17, 64, 64
  lens_l = [L, L - 40]
  q, w = inputs(2 * len(lens_l), Hi, dtype, 5, ints=True)
  k, table = cache(str(page), lens_l, dtype, 6, ints=True)
  lens = _i32(lens_l)
  got = ffpa_mla_index_scores(q, k, w, lens, table, max_seqlen_k=L)
  want, A = reference(q, k, w, lens, table, L)
  assert float(A.max()) * 4 < 2 ** 24  # (the sums stay exact in quarter units)
  assert torch.equal(got.cpu(), want.float())
  idx, n = ffpa_mla_sparse_topk_slots(got, topk, lens, table, page)
  want_idx, want_n = TR.topk_slots(want.float(), topk, lens.cpu(), table.cpu(), page)
  assert torch.equal(idx.cpu(), want_idx) and torch.equal(n.cpu(), want_n)


# ----------------------------------------------------------------------------- 3. one HIP graph
def test_one_graph_holds_scores_selection_and_the_sparse_call():
  """Captured once; cache_seqlens, the block table and the index-key pool are then rewritten in place: a replay returns what the eager calls return."""
  from ffpa_attn_amd import ffpa_attn_with_kvcache_mla_sparse, ffpa_mla_index_scores, ffpa_mla_sparse_topk_slots

  Hi, page, topk, N, lens_l = 64, 64, 96, C + 200, [C + 130, 70]
  q, w = inputs(4, Hi, torch.bfloat16, 7)
  k, table = cache(str(page), lens_l, torch.bfloat16, 8)
  g = torch.Generator(device="cuda").manual_seed(9)
  latent = torch.randn((k.size(0), page, 1, 576), generator=g, device="cuda", dtype=torch.bfloat16)
  ql = torch.randn((4, 16, 576), generator=g, device="cuda", dtype=torch.bfloat16)
  lens = _i32(lens_l)

  def step():
    s = ffpa_mla_index_scores(q, k, w, lens, table, max_seqlen_k=N)
    idx, n = ffpa_mla_sparse_topk_slots(s, topk, lens, table, page)
    return (s, idx, n) + ffpa_attn_with_kvcache_mla_sparse(ql, latent, 512, idx, topk_lens=n, softmax_scale=192 ** -0.5, num_splits=1, return_softmax_lse=True)

  step()  # (warm: the library is loaded, the scratch is sized)
  torch.cuda.synchronize()
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    held = step()
  for r, new_lens in enumerate((lens_l, [66, 128], [3, 0])):
    if r:
      k.copy_(torch.randn(k.shape, generator=g, device="cuda").to(k.dtype))
      table[:, :2] = table[:, :2].flip(1)  # (both sequences' first two pages are pages of theirs)
    lens.copy_(_i32(new_lens))
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(held, step()):
      assert torch.equal(a, b), new_lens
    want, A = reference(q, k, w, lens, table, N)
    check(held[0], want, A, Hi, f"replay {r}")
