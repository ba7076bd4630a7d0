"""``ffpa_mla_sparse_topk_slots`` / ``ffpa_mla_sparse_slots`` on the GPU past one step of the kernel's ordered pass, against their definition
(tests/kvcache_mla_sparse_topk_ref.py on the CPU copy of the same tensors): integer tensors, every comparison exact.  The cases and the conditions that keep them
from being vacuous are tests/kvcache_mla_sparse_topk_cases.py's — asserted again here in front of every launch: the placed rows (ties on the step edges, `need`
used up on a step's last column, ties only behind the first step, larger keys only in the last one, a field of ties, NaN / -inf / mixed zeros as the tie value,
one to four radix passes over three histogram bases, topk past a step with and without a table, the positions mode past a step, 257 sequences) and the 48 seeds
of the sweep.  Then the pair of a bf16-rounded 32k row feeding the sparse call, one HIP graph replayed at a three-step shape, and the C export on raw pointers
with ``indices_stride > topk`` between guard words."""

import ctypes

import pytest
import torch

import kvcache_mla_sparse_topk_cases as C
import kvcache_mla_sparse_topk_ref as TR
from test_fwd_gpu import hip  # noqa: F401  (fixture)
from test_kvcache_mla_sparse_topk_gpu import DV, D, SCALE, _pool, _same

pytestmark = pytest.mark.gpu

SENTINEL, GUARD = -777, 64


def _dev(x):
  """A CPU tensor of a case on the GPU, in its own layout: a view of a wider storage stays one (what lies outside the row travels too)."""
  if x is None or x.dim() < 2 or x.stride(0) == x.size(1):
    return None if x is None else x.cuda()
  return torch.as_strided(x, (x.size(0), x.stride(0)), (x.stride(0), 1), x.storage_offset()).cuda()[:, : x.size(1)]


def _run(case):
  """The case's conditions, then its public call against the definition, exactly."""
  from ffpa_attn_amd import ffpa_mla_sparse_slots

  C.conditions(case)
  lens, table, cu = case["cache_seqlens"].cuda(), _dev(case["block_table"]), _dev(case["cu_seqlens_q"])
  if case["scores"] is not None:
    scores = _dev(case["scores"])
    assert scores.stride() == case["scores"].stride() and (table is None or table.stride() == case["block_table"].stride())
    return _same(scores, case["topk"], lens, table, case["page_size"], cu, case["causal"], what=case["name"])
  pos = _dev(case["positions"])
  idx, n = ffpa_mla_sparse_slots(pos, lens, table, case["page_size"], cu_seqlens_q=cu)
  torch.cuda.synchronize()
  want_idx, want_n = TR.slots(case["positions"], case["cache_seqlens"], case["block_table"], case["page_size"], cu_seqlens_q=case["cu_seqlens_q"])
  assert idx.shape == want_idx.shape and idx.dtype == n.dtype == torch.int32 and idx.is_contiguous()
  assert torch.equal(n.cpu(), want_n), f"{case['name']}: counts {n.tolist()} != {want_n.tolist()}"
  bad = (idx.cpu() != want_idx).nonzero()
  assert bad.numel() == 0, f"{case['name']}: {bad.size(0)} entries differ, first at {bad[0].tolist()}: {int(idx[tuple(bad[0])])} != {int(want_idx[tuple(bad[0])])}"
  return idx, n


# ----------------------------------------------------------------------------- 1. the placed cases, 2. the sweep
@pytest.mark.parametrize("group", list(C.PLACED))
def test_a_placed_group(hip, group):
  for case in C.PLACED[group]():
    _run(case)


@pytest.mark.parametrize("seed", C.SEEDS)
def test_a_sweep_seed(hip, seed):
  _run(C.sweep_case(seed))


# ----------------------------------------------------------------------------- 3. end to end
def test_a_bf16_rounded_32k_row_feeds_the_sparse_call(hip):
  """What a 16-bit indexer hands over (``.float()``): dozens of keys equal the rank-2048 threshold, over all four steps.  O and LSE of the sparse call fed the
  kernel's pair are, bit for bit, those of the same call fed the definition's pair."""
  from ffpa_attn_amd import ffpa_attn_with_kvcache_mla_sparse, ffpa_mla_sparse_topk_slots

  case = C.bf16_rounded_32k()
  C.conditions(case)
  scores, lens, topk, page = case["scores"], case["cache_seqlens"], case["topk"], case["page_size"]
  table = case["block_table"].cuda()
  pool = _pool(table.numel() + 3, page, 161)
  q = torch.randn((scores.size(0), 16, D), generator=torch.Generator(device="cuda").manual_seed(163), device="cuda", dtype=torch.bfloat16)
  idx, n = ffpa_mla_sparse_topk_slots(scores.cuda(), topk, lens.cuda(), table, page)
  out, lse = ffpa_attn_with_kvcache_mla_sparse(q, pool, DV, idx, topk_lens=n, softmax_scale=SCALE, return_softmax_lse=True)
  ref_idx, ref_n = TR.topk_slots(scores, topk, lens, table.cpu(), page)
  assert ref_n.tolist() == [topk] * 4 and torch.equal(n.cpu(), ref_n) and torch.equal(idx.cpu(), ref_idx)
  want, want_lse = ffpa_attn_with_kvcache_mla_sparse(q, pool, DV, ref_idx.cuda(), topk_lens=ref_n.cuda(), softmax_scale=SCALE, return_softmax_lse=True)
  torch.cuda.synchronize()
  assert torch.equal(out, want) and torch.equal(lse, want_lse) and torch.isfinite(lse).all()


# ----------------------------------------------------------------------------- 4. one graph at a three-step shape
def test_one_graph_replayed_at_a_three_step_shape(hip):
  """N = 24581, topk = 8193, page 16.  Captured once on a single stream; the scores are then rewritten in place — the step-edges row, a bf16-rounded row, an
  all-equal row — and every replay equals the definition."""
  from ffpa_attn_amd import ffpa_mla_sparse_topk_slots

  fills = C.graph_fills()
  N, topk, page = C.N3, fills[0]["topk"], fills[0]["page_size"]
  table, lens = _dev(fills[0]["block_table"]), fills[0]["cache_seqlens"].cuda()
  scores = torch.randn(2, N, generator=torch.Generator().manual_seed(172)).cuda()
  ffpa_mla_sparse_topk_slots(scores, topk, lens, table, page)  # (warm: the library is loaded)
  torch.cuda.synchronize()
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    idx_g, n_g = ffpa_mla_sparse_topk_slots(scores, topk, lens, table, page)
  for case in fills:
    C.conditions(case)
    scores.copy_(case["scores"])
    graph.replay()
    torch.cuda.synchronize()
    want_idx, want_n = TR.topk_slots(case["scores"], topk, lens.cpu(), table.cpu(), page)
    assert torch.equal(n_g.cpu(), want_n) and torch.equal(idx_g.cpu(), want_idx), case["name"]


# ----------------------------------------------------------------------------- 5. the export on raw pointers
def _export(hip, rows, by_score, topk, lens, table, page, cu, causal):
  """``ffpa_attn_mla_sparse_topk_slots`` with ``indices_stride = topk + 7``, the whole output storage and GUARD words on either side of it pre-filled with
  SENTINEL, ``topk_lens`` guarded the same way -> (the [T, topk + 7] body, its guards, the T counts, their guards)."""
  lib = hip.load_library()
  T, stride = rows.size(0), topk + 7
  out = torch.full((GUARD + T * stride + GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
  cnt = torch.full((GUARD + T + GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
  p = hip._stamped(hip.FfpaMlaSparseTopkParams)
  if by_score:
    p.scores = rows.data_ptr()
  else:
    p.positions = rows.data_ptr()
  p.cache_seqlens, p.indices, p.topk_lens = lens.data_ptr(), out.data_ptr() + 4 * GUARD, cnt.data_ptr() + 4 * GUARD
  if cu is not None:
    p.cu_seqlens_q = cu.data_ptr()
  if table is not None:
    p.block_table, p.block_table_stride, p.W, p.page_size = table.data_ptr(), table.stride(0), table.size(1), page
  p.row_stride, p.indices_stride = rows.stride(0), stride
  p.T, p.N_or_topk, p.topk, p.B, p.causal = T, rows.size(1), topk, lens.numel(), int(causal)
  rc = hip._call_on_stream(lib.ffpa_attn_mla_sparse_topk_slots, rows.device, ctypes.byref(p))
  assert rc == 0, lib.ffpa_attn_last_error()
  torch.cuda.synchronize()
  out, cnt = out.cpu(), cnt.cpu()
  return out[GUARD:-GUARD].view(T, stride), torch.cat([out[:GUARD], out[-GUARD:]]), cnt[GUARD:-GUARD], torch.cat([cnt[:GUARD], cnt[-GUARD:]])


EXPORT_CASES = {"scores (24581, 8193)": lambda: C.topk_past_a_step(C.N3, C.S + 1)[4], "scores (1000, 100)": lambda: C.many_sequences()[0],
                "positions 8193": lambda: C.positions_past_a_step(C.S + 1)[0]}


@pytest.mark.parametrize("which", list(EXPORT_CASES))
def test_the_export_with_a_padded_indices_stride(hip, which):
  """The topk columns of every row equal the definition; every padding column, every guard word around ``indices`` and around the T entries of ``topk_lens``
  still holds the sentinel."""
  case = EXPORT_CASES[which]()
  C.conditions(case)
  by_score = case["scores"] is not None
  assert (by_score, case["topk"], case["block_table"] is not None) == {"scores (24581, 8193)": (True, C.S + 1, True), "scores (1000, 100)": (True, 100, False),
                                                                        "positions 8193": (False, C.S + 1, True)}[which]
  rows = case["scores"] if by_score else case["positions"]
  table, cu, lens, topk = case["block_table"], case["cu_seqlens_q"], case["cache_seqlens"], case["topk"]
  if by_score:
    want_idx, want_n = TR.topk_slots(rows, topk, lens, table, case["page_size"], cu_seqlens_q=cu, causal=case["causal"])
  else:
    want_idx, want_n = TR.slots(rows, lens, table, case["page_size"], cu_seqlens_q=cu)
  assert (want_idx == SENTINEL).sum() == 0
  body, guards, counts, count_guards = _export(hip, _dev(rows), by_score, topk, lens.cuda(), _dev(table), case["page_size"] or 0, _dev(cu), case["causal"])
  assert torch.equal(counts, want_n), which
  bad = (body[:, :topk] != want_idx).nonzero()
  assert bad.numel() == 0, f"{which}: {bad.size(0)} entries differ, first at {bad[0].tolist()}"
  assert (body[:, topk:] == SENTINEL).all() and (guards == SENTINEL).all() and (count_guards == SENTINEL).all(), which
