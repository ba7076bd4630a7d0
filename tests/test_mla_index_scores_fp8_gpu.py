"""``ffpa_mla_index_scores_fp8`` and ``ffpa_mla_index_k_append_fp8`` on the GPU.  The scores against their definition in float64 on the very codes and scales: the
WHOLE ``[T, N]`` tensor, -inf columns exactly -inf, a finite column within ``(128 + Hi + 9) * 2^-23 * A[t, p]``, ``A = kscale * sum_h |w| sum_d |q8 k8|`` — the
16-bit call's derived fp32 worst case (128 products and Hi weighted terms in any order, chopped or rounded) with one more rounding for the key scale; derived, not
measured: it models the FP8 MFMA's 128-term sum as fp32 adds.  Then integer codes bit for bit into the selection, the token rules, the append byte for byte
against ``quantize_index_rows`` + ``pack_index_key_pages``, and the four launches append -> scores -> selection -> sparse attention in one HIP graph."""

import pytest
import torch

import kvcache_mla_sparse_topk_ref as TR
from ffpa_attn_amd import pack_index_key_pages, quantize_index_rows, unpack_index_key_pages
from ffpa_attn_amd.hip import MLA_INDEX_CHUNK_KEYS as C
from test_fwd_gpu import hip  # noqa: F401  (fixture)
from test_mla_index_scores_gpu import LENGTHS, NINF, _i32, cache, inputs, reference

pytestmark = pytest.mark.gpu

E4M3 = torch.float8_e4m3fn


def check(got, want, A, Hi, what=""):
  got = got.cpu()
  assert got.dtype == torch.float32 and got.shape == want.shape and got.is_contiguous()
  tail = want == NINF
  assert torch.equal(got == NINF, tail), f"{what}: the -inf columns differ in {int(((got == NINF) != tail).sum())} places"
  err, a = (got.double() - want)[~tail].abs(), A[~tail].clamp(min=1e-300)
  print(f"{what}: worst err / A = {float((err / a).max()) if err.numel() else 0.0:.3e} (allowed {(128 + Hi + 9) * 2.0 ** -23:.3e})")
  assert bool((err <= (128 + Hi + 9) * 2.0 ** -23 * a).all()), f"{what}: {int((err > (128 + Hi + 9) * 2.0 ** -23 * a).sum())} columns past the bound"


def q8_of(T, Hi, seed, strided=False, ints=False):
  """-> ``(q_index e4m3, weights)``: ``inputs``'s values as codes (integers convert exactly); ``strided``: a view with a storage offset, strides multiples of 16."""
  q, w = inputs(T, Hi, torch.bfloat16, seed, strided=strided, ints=ints)
  codes = q.to(E4M3) if ints else quantize_index_rows(q)[0]
  if strided:
    store = torch.zeros((T + 1, Hi + 1, 144), dtype=E4M3, device="cuda")
    store[1:, 1:, 16:] = codes
    codes = store[1:, 1:, 16:]
  return codes, w


def pool(layout, lens, seed, scales="pow2", ints=False, spare=2):
  """-> ``(k_index_cache uint8, block_table | None, the keys' values float64 [pages, page_size, 128])``: ``cache``'s pool and table with its values as codes and
  a scale that DIFFERS per key — powers of two over 2^-8 ... 2^3, arbitrary positive floats, or {1/2, 1, 2}."""
  k, table = cache(layout, lens, torch.bfloat16, seed, ints=ints, spare=spare)
  k = k.reshape(k.size(0), k.size(1), 128)
  codes = k.to(E4M3) if ints else quantize_index_rows(k)[0]
  g = torch.Generator(device="cuda").manual_seed(seed + 100)
  lo, hi = (-1, 2) if ints else (-8, 4)
  scale = 2.0 ** torch.randint(lo, hi, k.shape[:2], generator=g, device="cuda").float()
  if scales == "any":
    scale = scale * (1 + torch.rand(k.shape[:2], generator=g, device="cuda"))
  pages = pack_index_key_pages(codes, scale)
  return (pages.unsqueeze(2) if layout == "64" else pages), table, codes.cpu().double() * scale.cpu().double()[..., None]


# ----------------------------------------------------------------------------- 1. against float64
@pytest.mark.parametrize("scales", ["pow2", "any"])
@pytest.mark.parametrize("layout", ["64", "128", "contiguous"])
@pytest.mark.parametrize("Hi", [32, 64])
def test_every_length_against_float64(Hi, layout, scales):
  """One token per sequence, one sequence per length of LENGTHS, N past the longest; table ids far outside the pool behind every sequence's last page."""
  from ffpa_attn_amd import ffpa_mla_index_scores_fp8

  N = max(LENGTHS) + 30
  q, w = q8_of(len(LENGTHS), Hi, 1)
  k, table, kval = pool(layout, LENGTHS, 2, scales)
  got = ffpa_mla_index_scores_fp8(q, k, w, _i32(LENGTHS), table, max_seqlen_k=N)
  want, A = reference(q.float(), kval, w, _i32(LENGTHS), table, N)
  assert [int((r != NINF).sum()) for r in want] == LENGTHS
  check(got, want, A, Hi, f"Hi {Hi} {layout} {scales}")


# ----------------------------------------------------------------------------- 2. exact, and end to end
def test_integer_codes_are_exact_and_feed_the_selection():
  """Codes in [-3, 3], key scales in {1/2, 1, 2}, weights +-{1/4, 1/2, 1, 2}: every operation is exact in any order, so the scores EQUAL the float64
  definition — a wrong format code or A / B column mappings that differ cannot pass — and the selection over them equals the reference selection."""
  from ffpa_attn_amd import ffpa_mla_index_scores_fp8, ffpa_mla_sparse_topk_slots

  Hi, L, page, topk = 64, 2 * C + 17, 64, 64
  lens_l = [L, L - 40]
  q, w = q8_of(2 * len(lens_l), Hi, 5, ints=True)
  k, table, kval = pool(str(page), lens_l, 6, ints=True)
  lens = _i32(lens_l)
  got = ffpa_mla_index_scores_fp8(q, k, w, lens, table, max_seqlen_k=L)
  want, A = reference(q.float(), kval, w, lens, table, L)
  assert float(A.max()) * 8 < 2 ** 24  # (the sums stay exact in eighth units)
  assert torch.equal(got.cpu(), want.float())
  idx, n = ffpa_mla_sparse_topk_slots(got, topk, lens, table, page)
  want_idx, want_n = TR.topk_slots(want.float(), topk, lens.cpu(), table.cpu(), page)
  assert torch.equal(idx.cpu(), want_idx) and torch.equal(n.cpu(), want_n)


# ----------------------------------------------------------------------------- 3. the token rules
@pytest.mark.parametrize("case, Hi, layout", [("causal3", 64, "64"), ("noncausal3", 32, "128"), ("clamp", 32, "contiguous"), ("ragged", 64, "64"),
                                              ("table_inside", 32, "128"), ("table_short", 64, "64"), ("table_short", 32, "contiguous")])
def test_token_rules_against_float64(case, Hi, layout):
  """Sq = 3 causal (tokens whose n_t is <= 0 included) and non-causal; N below the lengths; a ragged step with an empty sequence, padding rows and strided
  q_index / weights; a page id outside the pool INSIDE a sequence (clamped); a table / a capacity too small for the lengths."""
  from ffpa_attn_amd import ffpa_mla_index_scores_fp8

  lens_l, cu, causal, N = [1, 2, 65, C + 1, 2 * C + 17, 0], None, case != "noncausal3", 2 * C + 80
  T = 3 * len(lens_l)
  if case == "clamp":
    N = C - 3
  elif case == "ragged":
    cu, T = _i32([0, 2, 2, 7, 8, 9, 9]), 12  # (sequence 1 and 5 have no token; rows 9 ... 11 are padding)
  q, w = q8_of(T, Hi, 3, strided=case == "ragged")
  k, table, kval = pool(layout, lens_l, 4, "any", spare=0 if case == "table_short" else 2)
  lens = _i32(lens_l)
  if case == "table_inside":
    table[4, 1], table[3, 0] = 10 ** 9, -5
  if case == "table_short":
    lens = lens + 300  # (lengths past what the table / the capacity can name: n_t stops there)
  got = ffpa_mla_index_scores_fp8(q, k, w, lens, table, max_seqlen_k=N, cu_seqlens_q=cu, causal=causal)
  want, A = reference(q.float(), kval, w, lens, table, N, cu, causal)
  if case == "causal3":
    assert bool((want[0] == NINF).all()) and bool((want[2, :1] != NINF).all())  # (token 0 of 3 of a sequence of length 1 sees nothing)
  check(got, want, A, Hi, f"{case} Hi {Hi} {layout}")


# ----------------------------------------------------------------------------- 4. the append
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("layout", ["64", "contiguous"])
@pytest.mark.parametrize("ragged", [False, True])
def test_append_writes_the_bytes_of_the_torch_definition(ragged, layout, dtype):
  """Sequences at length 0, ending mid-page, crossing a page, passing the capacity (192 keys) and at a negative length (acts as 0); an all-zero row, a row whose
  amax is exactly 2^-3 * 448 and one just above; ragged: a sequence without a row and padding rows.  The WHOLE pool equals the expectation, sentinel included."""
  from ffpa_attn_amd import ffpa_mla_index_k_append_fp8

  page, W, B, before = 64, 3, 5, [0, 20, 60, 190, -3]
  counts = [6, 0, 7, 5, 2] if ragged else [6] * B
  T = sum(counts) + (3 if ragged else 0)
  g = torch.Generator(device="cuda").manual_seed(11)
  x = (torch.randn((T, 1, 128), generator=g, device="cuda") * 3).to(dtype)
  x[0] = 0
  x[1, 0, 5], x[2, 0, 7] = 56.0, -56.25  # (the largest of their rows: randn * 3 stays far below)
  if layout == "64":
    ids = torch.randperm(B * W + 2, generator=torch.Generator().manual_seed(12))[:B * W].view(B, W)
    table, pages_n, ps = ids.to(torch.int32).cuda(), B * W + 2, page
  else:
    ids, table, pages_n, ps = torch.arange(B).view(B, 1), None, B, W * page
  k = torch.full((pages_n, ps, 132), 0xA5, dtype=torch.uint8, device="cuda")
  codes, scale = unpack_index_key_pages(k.cpu())
  new_codes, new_scale = quantize_index_rows(x[:, 0].cpu())
  assert new_scale[:3].tolist() == [2.0 ** -22, 2.0 ** -3, 2.0 ** -2] and new_codes[1, 5].float() == 448
  t = 0
  for b in range(B):
    for i in range(counts[b]):
      pos = max(before[b], 0) + i
      if pos < W * page:
        codes[ids[b, pos // ps], pos % ps], scale[ids[b, pos // ps], pos % ps] = new_codes[t], new_scale[t]
      t += 1
  cu = _i32([0] + torch.tensor(counts).cumsum(0).tolist()) if ragged else None
  after = ffpa_mla_index_k_append_fp8(k.unsqueeze(2) if layout == "64" else k, x if ragged else x[:, 0], _i32(before), table, cu_seqlens_q=cu)
  assert after.dtype == torch.int32 and after.tolist() == [min(max(L, 0) + c, W * page) for L, c in zip(before, counts)]
  assert torch.equal(k.cpu(), pack_index_key_pages(codes, scale))


# ----------------------------------------------------------------------------- 5. one HIP graph
def test_one_graph_holds_append_scores_selection_and_the_sparse_call():
  """Captured once; k_index, cache_seqlens and the block table are then rewritten in place: a replay returns what the eager calls return."""
  from ffpa_attn_amd import ffpa_attn_with_kvcache_mla_sparse, ffpa_mla_index_k_append_fp8, ffpa_mla_index_scores_fp8, ffpa_mla_sparse_topk_slots

  Hi, page, topk, N, lens_l = 64, 64, 96, C + 200, [C + 130, 70]
  q, w = q8_of(4, Hi, 7)
  k, table, _ = pool(str(page), [L + 2 for L in lens_l], 8)
  g = torch.Generator(device="cuda").manual_seed(9)
  latent = torch.randn((k.size(0), page, 1, 576), generator=g, device="cuda", dtype=torch.bfloat16)
  ql = torch.randn((4, 16, 576), generator=g, device="cuda", dtype=torch.bfloat16)
  k_new = torch.randn((4, 128), generator=g, device="cuda", dtype=torch.bfloat16)
  lens = _i32(lens_l)

  def step():
    after = ffpa_mla_index_k_append_fp8(k, k_new, lens, table)
    s = ffpa_mla_index_scores_fp8(q, k, w, after, table, max_seqlen_k=N)
    idx, n = ffpa_mla_sparse_topk_slots(s, topk, after, table, page)
    return (after, s, idx, n) + ffpa_attn_with_kvcache_mla_sparse(ql, latent, 512, idx, topk_lens=n, softmax_scale=192 ** -0.5, num_splits=1, return_softmax_lse=True)

  step()  # (warm: the library is loaded, the scratch is sized)
  torch.cuda.synchronize()
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    held = step()
  for r, new_lens in enumerate((lens_l, [66, 126], [3, 0])):
    if r:
      k_new.copy_(torch.randn(k_new.shape, generator=g, device="cuda").to(k_new.dtype))
      table[:, :2] = table[:, :2].flip(1)  # (both sequences' first two pages are pages of theirs)
    lens.copy_(_i32(new_lens))
    graph.replay()
    torch.cuda.synchronize()
    assert held[0].tolist() == [L + 2 for L in new_lens]
    for a, b in zip(held, step()):
      assert torch.equal(a, b), new_lens
    codes, scale = unpack_index_key_pages(k[:, :, 0].cpu())
    want, A = reference(q.float(), codes.double() * scale.double()[..., None], w, held[0], table, N)
    check(held[1], want, A, Hi, f"replay {r}")
