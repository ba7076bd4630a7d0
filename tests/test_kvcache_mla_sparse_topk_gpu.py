"""``ffpa_mla_sparse_topk_slots`` / ``ffpa_mla_sparse_slots`` on the GPU against their definition (tests/kvcache_mla_sparse_topk_ref.py, run on the CPU copy of the
same tensors): integer tensors, every comparison exact.  Lengths, ties and radix digits, token -> sequence, the translation, the positions mode against the two
torch helpers, the pair feeding the sparse call (and the dense latent call's bits where every key is selected), one HIP graph, ``torch.compile``.

Ties, special values and all four radix passes are run here at 4097 columns — ONE step of the kernel's ordered pass (8192 columns), one histogram base —, and no
``topk`` here passes 4096.  The multi-step cases — ties carried over step edges, ``topk`` and the positions mode past 8192, several histogram bases, 257 sequences,
``indices_stride > topk`` through the C export — live in tests/test_kvcache_mla_sparse_topk_sweep_gpu.py, their builders and conditions in
tests/kvcache_mla_sparse_topk_cases.py."""

import pytest
import torch

import kvcache_mla_sparse_topk_ref as TR
from test_fwd_gpu import hip  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

D, DV = 576, 512
SCALE = 192 ** -0.5
NAN, INF = float("nan"), float("inf")


def _i32(x):
  return torch.tensor(x, dtype=torch.int32, device="cuda")


def _cpu(t):
  return None if t is None else t.cpu()


def _same(scores, topk, lens, table=None, page=None, cu=None, causal=True, what=""):
  """The call's pair equals the definition's on the same tensors, exactly -> the pair."""
  from ffpa_attn_amd import ffpa_mla_sparse_topk_slots

  idx, n = ffpa_mla_sparse_topk_slots(scores, topk, lens, table, page, cu_seqlens_q=cu, causal=causal)
  torch.cuda.synchronize()
  want_idx, want_n = TR.topk_slots(scores.cpu(), topk, lens.cpu(), _cpu(table), page, cu_seqlens_q=_cpu(cu), causal=causal)
  assert idx.shape == want_idx.shape and idx.dtype == torch.int32 and idx.is_contiguous() and n.shape == want_n.shape and n.dtype == torch.int32
  assert torch.equal(n.cpu(), want_n), f"{what}: counts {n.tolist()} != {want_n.tolist()}"
  bad = (idx.cpu() != want_idx).nonzero()
  assert bad.numel() == 0, f"{what}: {bad.size(0)} entries differ, first at {bad[0].tolist()}: {int(idx[tuple(bad[0])])} != {int(want_idx[tuple(bad[0])])}"
  return idx, n


def _scores(T, N, seed, stride=None):
  """Random float32 scores [T, N]; with ``stride`` a view of a wider storage whose other columns hold NaN."""
  g = torch.Generator(device="cuda").manual_seed(seed)
  if stride is None:
    return torch.randn((T, N), generator=g, device="cuda")
  store = torch.full((T, stride), NAN, device="cuda")
  store[:, :N] = torch.randn((T, N), generator=g, device="cuda")
  return store[:, :N]


# ----------------------------------------------------------------------------- 1. lengths
@pytest.mark.parametrize("N, topk", [(1000, 1), (1000, 100), (1000, 1000), (4097, 1), (4097, 100), (4097, 2048), (8192, 2048)])
def test_visible_lengths_around_topk_and_the_row(N, topk):
  """n = 0, 1, topk - 1, topk, topk + 1, N, a length above N and a negative one — one sequence of one token each.  What stands at and past n is NaN (the largest
  key there is): never selected."""
  lens_l = [0, 1, topk - 1, topk, min(topk + 1, N), N, N + 77, -5]
  scores = _scores(len(lens_l), N, 10 + topk, stride=N + 13)
  for t, L in enumerate(lens_l):
    scores[t, max(min(L, N), 0):] = NAN
  idx, n = _same(scores, topk, _i32(lens_l), causal=True, what=f"N {N} topk {topk}")
  assert n.tolist() == [min(max(min(L, N), 0), topk) for L in lens_l]


def test_one_row_past_two_to_the_sixteen_columns():
  scores = _scores(1, 70000, 3)
  idx, n = _same(scores, 2048, _i32([70000]), what="70000 columns")
  assert int(n) == 2048 and int(idx[0, -1]) > 65536
  _same(scores, 2048, _i32([69999]), what="70000 columns, 69999 visible")


# ----------------------------------------------------------------------------- 2. ties and digits
@pytest.mark.parametrize("topk", [1, 100, 2048])
def test_ties_fill_the_threshold_bucket(topk):
  """Scores from {-2 ... 2} only (hundreds of equal keys at the threshold: the lower position wins), and an all-equal row."""
  g = torch.Generator(device="cuda").manual_seed(topk)
  scores = torch.randint(-2, 3, (4, 4097), generator=g, device="cuda").float()
  scores[3] = 0.5
  scores[2, ::2] = -0.0  # (-0.0 ties with +0.0)
  _same(scores, topk, _i32([4097, 4000, 4097, 4097]), what=f"ties, topk {topk}")


def test_all_four_radix_passes_and_the_special_values():
  """1 + i * 2^-23 in shuffled order: the keys differ in their last byte only after three shared ones.  And a row that mixes +-0.0, +-inf, denormals, negatives
  and three NaNs."""
  N = 4097
  g = torch.Generator().manual_seed(7)
  fine = (1 + torch.arange(N, dtype=torch.float64) * 2.0 ** -23).float()[torch.randperm(N, generator=g)]
  assert fine.unique().numel() == N
  mixed = torch.randn(N, generator=g)
  mixed[torch.randperm(N, generator=g)[:600]] = torch.tensor([0.0, -0.0, INF, -INF, 1e-45, -1e-45, 1e-39, -3e-39, -1.0, -7.5]).repeat(60)
  mixed[[5, 2000, 4096]] = NAN
  few = torch.full((N,), -INF)
  few[[1, 77, 4000]] = torch.tensor([-0.0, 1e-45, NAN])
  scores = torch.stack([fine, mixed, few, -fine]).cuda()
  for topk in (1, 3, 100, 700, 2048, 4096):
    _same(scores, topk, _i32([N] * 4), what=f"digits and specials, topk {topk}")


# ----------------------------------------------------------------------------- 3. token -> sequence
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("Sq", [1, 4])
def test_uniform_rows_of_a_b_by_sq_step(Sq, causal):
  B, N, topk = 2, 1000, 100
  _same(_scores(B * Sq, N, 20 + Sq), topk, _i32([102, 640]), causal=causal, what=f"[B, Sq = {Sq}] causal {causal}")


@pytest.mark.parametrize("causal", [True, False])
def test_ragged_rows_with_an_empty_sequence_and_padding(causal):
  """Sequences of 0, 1, 3 and 64 query tokens; three padding rows behind cu_seqlens_q[B] (count 0, a row of -1, whatever their scores hold)."""
  cu = _i32([0, 0, 1, 4, 68])
  scores = _scores(71, 1000, 31)
  scores[68:] = NAN
  lens = _i32([500, 7, 101, 130])  # (tokens 0 .. 2 of the third sequence see 99, 100, 101 columns under causal; the fourth's first ones 67, 68, ...)
  idx, n = _same(scores, 100, lens, cu=cu, causal=causal, what=f"ragged, causal {causal}")
  assert n[68:].tolist() == [0, 0, 0] and n[0].item() == 7 and n[1:4].tolist() == ([99, 100, 100] if causal else [100] * 3)


# ----------------------------------------------------------------------------- 4. the translation
@pytest.mark.parametrize("page", [1, 16, 64])
def test_a_shuffled_padded_block_table(page):
  """A shuffled table of W columns inside a wider storage (row stride > W, the rest far outside any pool); positions up to the last column of the table."""
  B, Sq, N = 3, 2, 1000
  W = -(-N // page)
  store = torch.full((B, W + 5), 2 ** 30, dtype=torch.int32, device="cuda")
  table = store[:, :W]
  table.copy_(torch.randperm(B * W + 9, generator=torch.Generator().manual_seed(page))[: B * W].view(B, W))
  idx, n = _same(_scores(B * Sq, N, 40 + page), 100, _i32([N, 640, 50]), table, page, what=f"page {page}")
  idx, n = _same(_scores(B * Sq, N, 40 + page), 1000, _i32([N, 640, 50]), table, page, what=f"page {page}, every position")
  assert int(idx[1, N - 1]) == int(table[0, W - 1]) * page + (N - 1) % page


def test_a_table_shorter_than_the_row_reads_its_last_column_and_none_writes_positions():
  scores = _scores(2, 1000, 50)
  table = torch.randperm(40, generator=torch.Generator().manual_seed(1))[:8].to(torch.int32).view(2, 4).cuda()
  _same(scores, 1000, _i32([1000, 999]), table, 64, what="W * page < N")
  idx, n = _same(scores, 1000, _i32([1000, 999]), what="no table")
  assert idx[0].tolist() == list(range(1000))


# ----------------------------------------------------------------------------- 5. the positions mode
@pytest.mark.parametrize("topk", [64, 100, 2048])
def test_positions_mode_is_the_two_helpers_in_one_launch(topk):
  """Holes at the front, in the middle, everywhere and nowhere; ragged rows with a padding row.  Against the definition, and — front entries and counts —
  against compact_topk_indices(slots_from_block_table(...)) fed a per-token table."""
  from ffpa_attn_amd import compact_topk_indices, ffpa_mla_sparse_slots, slots_from_block_table

  g = torch.Generator().manual_seed(topk)
  page, W, B = 16, 300, 3
  cu, seq = _i32([0, 2, 2, 7]), [0, 0, 2, 2, 2, 2, 2]
  pos = torch.randint(0, W * page + 40, (8, topk), generator=g, dtype=torch.int32)
  pos[0, : topk // 3] = -1
  pos[1, topk // 3: topk // 2] = -1
  pos[2][torch.rand(topk, generator=g) < 0.5] = -1
  pos[4], pos[5, 1:], pos[6, :-1] = -1, -1, -3
  pos = pos.cuda()
  table = torch.randperm(B * W, generator=g).to(torch.int32).view(B, W).cuda()
  lens = _i32([5, 5, 5])
  for tb, pg in ((table, page), (None, None)):
    idx, n = ffpa_mla_sparse_slots(pos, lens, tb, pg, cu_seqlens_q=cu)
    torch.cuda.synchronize()
    want_idx, want_n = TR.slots(pos.cpu(), lens.cpu(), _cpu(tb), pg, cu_seqlens_q=cu.cpu())
    assert torch.equal(n.cpu(), want_n) and torch.equal(idx.cpu(), want_idx) and idx.dtype == n.dtype == torch.int32
    live = pos[:7] if tb is None else slots_from_block_table(pos[:7], tb[seq], pg)
    h_idx, h_n = compact_topk_indices(live)
    front = torch.arange(topk, device="cuda")[None] < h_n[:, None]
    assert torch.equal(n[:7], h_n) and torch.equal(idx[:7][front], h_idx[front]) and int(n[7]) == 0 and (idx[7] == -1).all()


# ----------------------------------------------------------------------------- 6. end to end
def _pool(pages, page, seed):
  g = torch.Generator(device="cuda").manual_seed(seed)
  return torch.randn((pages, page, 1, D), generator=g, device="cuda", dtype=torch.bfloat16)


def test_the_pair_feeds_the_sparse_call():
  from ffpa_attn_amd import ffpa_attn_with_kvcache_mla_sparse, ffpa_mla_sparse_topk_slots

  B, Sq, N, topk, page = 2, 2, 1000, 96, 16
  W = -(-N // page)
  pool = _pool(B * W + 3, page, 60)
  table = torch.randperm(B * W + 3, generator=torch.Generator().manual_seed(2))[: B * W].to(torch.int32).view(B, W).cuda()
  scores, lens = _scores(B * Sq, N, 61), _i32([1000, 70])
  q = torch.randn((B * Sq, 16, D), generator=torch.Generator(device="cuda").manual_seed(62), device="cuda", dtype=torch.bfloat16)
  idx, n = ffpa_mla_sparse_topk_slots(scores, topk, lens, table, page)
  out, lse = ffpa_attn_with_kvcache_mla_sparse(q, pool, DV, idx, topk_lens=n, softmax_scale=SCALE, return_softmax_lse=True)
  ref_idx, ref_n = TR.topk_slots(scores.cpu(), topk, lens.cpu(), table.cpu(), page)
  assert ref_n.tolist() == [96, 96, 69, 70]
  want, want_lse = ffpa_attn_with_kvcache_mla_sparse(q, pool, DV, ref_idx.cuda(), topk_lens=ref_n.cuda(), softmax_scale=SCALE, return_softmax_lse=True)
  torch.cuda.synchronize()
  assert torch.equal(out, want) and torch.equal(lse, want_lse) and torch.isfinite(lse).all()


def test_every_key_selected_is_the_dense_latent_call_to_the_bit():
  """n <= topk everywhere and topk % 32 == 0: the row lists the sequence's slots in order and the sparse call returns the dense latent call's bits (bf16 O, LSE)."""
  from ffpa_attn_amd import ffpa_attn_with_kvcache_mla, ffpa_attn_with_kvcache_mla_sparse, ffpa_mla_sparse_topk_slots

  lens_l, page, pps = [1, 33, 64, 97, 300, 0], 64, 5
  T, topk = len(lens_l), 320
  pool = _pool(T * pps + 1, page, 70)
  table = torch.randperm(T * pps + 1, generator=torch.Generator().manual_seed(3))[: T * pps].to(torch.int32).view(T, pps).cuda()
  lens = _i32(lens_l)
  q = torch.randn((T, 16, D), generator=torch.Generator(device="cuda").manual_seed(71), device="cuda", dtype=torch.bfloat16)
  idx, n = ffpa_mla_sparse_topk_slots(_scores(T, pps * page, 72), topk, lens, table, page)
  assert n.tolist() == lens_l
  out, lse = ffpa_attn_with_kvcache_mla_sparse(q, pool, DV, idx, topk_lens=n, softmax_scale=SCALE, num_splits=1, return_softmax_lse=True)
  want, want_lse = ffpa_attn_with_kvcache_mla(q[:, None], pool, DV, cache_seqlens=lens, block_table=table, softmax_scale=SCALE, num_splits=1, return_softmax_lse=True)
  torch.cuda.synchronize()
  assert torch.equal(lse, want_lse[:, :, 0].t()) and torch.equal(out, want[:, 0])


# ----------------------------------------------------------------------------- 7. one graph, torch.compile
def test_one_graph_holds_the_selection_and_the_sparse_call():
  """Captured once on a single stream; scores, cache_seqlens and the block table are then rewritten in place: every replay equals the definition's pair and the
  sparse call fed by it."""
  from ffpa_attn_amd import ffpa_attn_with_kvcache_mla_sparse, ffpa_mla_sparse_topk_slots

  B, Sq, N, topk, page = 2, 2, 1000, 96, 16
  W = -(-N // page)
  pool = _pool(B * W, page, 80)
  gc = torch.Generator().manual_seed(4)
  table = torch.randperm(B * W, generator=gc).to(torch.int32).view(B, W).cuda()
  scores, lens = _scores(B * Sq, N, 81), _i32([1000, 70])
  q = torch.randn((B * Sq, 16, D), generator=torch.Generator(device="cuda").manual_seed(82), device="cuda", dtype=torch.bfloat16)

  def step():
    idx, n = ffpa_mla_sparse_topk_slots(scores, topk, lens, table, page)
    return (idx, n) + ffpa_attn_with_kvcache_mla_sparse(q, pool, DV, idx, topk_lens=n, softmax_scale=SCALE, num_splits=1, return_softmax_lse=True)

  step()  # (warm: the library is loaded, the scratch is sized)
  torch.cuda.synchronize()
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    idx_g, n_g, out_g, lse_g = step()
  for k, lens_l in enumerate(([1000, 70], [3, 999], [97, 0])):
    if k:
      scores.copy_(_scores(B * Sq, N, 83 + k))
      table.copy_(torch.randperm(B * W, generator=gc).to(torch.int32).view(B, W))
    lens.copy_(_i32(lens_l))
    graph.replay()
    torch.cuda.synchronize()
    want_idx, want_n = TR.topk_slots(scores.cpu(), topk, lens.cpu(), table.cpu(), page)
    assert torch.equal(idx_g.cpu(), want_idx) and torch.equal(n_g.cpu(), want_n), lens_l
    want, want_lse = ffpa_attn_with_kvcache_mla_sparse(q, pool, DV, want_idx.cuda(), topk_lens=want_n.cuda(), softmax_scale=SCALE, num_splits=1, return_softmax_lse=True)
    torch.cuda.synchronize()
    assert torch.equal(out_g, want) and torch.equal(lse_g, want_lse), lens_l


def test_under_torch_compile_fullgraph():
  from ffpa_attn_amd import ffpa_attn_with_kvcache_mla_sparse, ffpa_mla_sparse_slots, ffpa_mla_sparse_topk_slots

  B, N, topk, page = 2, 1000, 96, 16
  W = -(-N // page)
  pool = _pool(B * W, page, 90)
  table = torch.randperm(B * W, generator=torch.Generator().manual_seed(5)).to(torch.int32).view(B, W).cuda()
  scores, lens = _scores(B, N, 91), _i32([1000, 70])
  q = torch.randn((B, 16, D), generator=torch.Generator(device="cuda").manual_seed(92), device="cuda", dtype=torch.bfloat16)

  def f(q, pool, scores, lens, table):
    idx, n = ffpa_mla_sparse_topk_slots(scores, topk, lens, table, page)
    pos, _ = ffpa_mla_sparse_topk_slots(scores, topk, lens)
    idx2, n2 = ffpa_mla_sparse_slots(pos, lens, table, page)
    o, lse = ffpa_attn_with_kvcache_mla_sparse(q, pool, DV, idx, topk_lens=n, softmax_scale=SCALE, return_softmax_lse=True)
    return o * 2, lse, idx, n, idx2, n2

  eager = f(q, pool, scores, lens, table)
  compiled = torch.compile(f, fullgraph=True)(q, pool, scores, lens, table)
  torch.cuda.synchronize()
  for e, c in zip(eager, compiled):
    assert torch.equal(e, c)
  want_idx, want_n = TR.topk_slots(scores.cpu(), topk, lens.cpu(), table.cpu(), page)
  assert torch.equal(compiled[2].cpu(), want_idx) and torch.equal(compiled[3].cpu(), want_n)
  assert torch.equal(compiled[4], compiled[2]) and torch.equal(compiled[5], compiled[3])  # (the positions mode over the selection's own positions: the same pair)
