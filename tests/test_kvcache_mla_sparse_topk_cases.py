"""The cases of tests/kvcache_mla_sparse_topk_cases.py without a GPU: the builders are deterministic, every placed case meets its conditions, the seeded sweep's
census holds, and the definition on three of the placed rows equals a brute-force selection.  tests/test_kvcache_mla_sparse_topk_sweep_gpu.py runs the same cases
on the GPU."""

import numpy as np
import pytest
import torch

import kvcache_mla_sparse_topk_cases as C
import kvcache_mla_sparse_topk_ref as TR

TENSORS = ("scores", "positions", "cache_seqlens", "block_table", "cu_seqlens_q")


def _identical(a, b):
  """Two builds of one case: the same arguments, and the same bits in the same layout (NaN and -0.0 included)."""
  assert a["name"] == b["name"] and a["topk"] == b["topk"] and a["page_size"] == b["page_size"] and a["causal"] == b["causal"]
  for k in TENSORS:
    x, y = a[k], b[k]
    assert (x is None) == (y is None), k
    if x is not None:
      assert x.dtype == y.dtype and x.shape == y.shape and x.stride() == y.stride() and x is not y, (a["name"], k)
      assert torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32)), (a["name"], k)


def test_the_constants_are_the_kernels():
  """kThreads, kPer and kSpan as csrc/ffpa_mla_sparse_topk.hip states them."""
  import os
  import re

  src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ffpa_attn_amd", "csrc", "ffpa_mla_sparse_topk.hip")).read()
  threads, per = (int(re.search(rf"constexpr int {name} = (\d+);", src).group(1)) for name in ("kThreads", "kPer"))
  assert "constexpr int kSpan = kThreads * kPer;" in src
  assert (C.THREADS, C.PIECE, C.SEG, C.S) == (threads, 64, 64 * per, threads * per) and C.N3 == 3 * C.S + 5


@pytest.mark.parametrize("group", list(C.PLACED))
def test_a_placed_group_is_deterministic_and_meets_its_conditions(group):
  cases, again = C.PLACED[group](), C.PLACED[group]()
  assert len(cases) == len(again) >= 1 and len({c["name"] for c in cases}) == len(cases)
  for a, b in zip(cases, again):
    _identical(a, b)
    assert a["check"] is not None, a["name"]
    C.conditions(a)


def test_the_end_to_end_and_the_graph_cases_meet_their_conditions():
  for case, again in zip([C.bf16_rounded_32k()] + C.graph_fills(), [C.bf16_rounded_32k()] + C.graph_fills()):
    _identical(case, again)
    C.conditions(case)


def test_the_placed_groups_hold_the_cases_they_are_meant_to():
  names = [c["name"] for group in ("step edges", "need ends a step", "ties behind the first step", "tie field", "special tie values", "radix depth") for c in C.PLACED[group]()]
  assert len(names) == 6 + 2 + 2 + len(C.FIELD_NEEDS) + 4 + 4
  assert {1, 63, 64, 65, 511, 512, 513, C.S - 6, C.S - 5, C.S - 4, C.S + 1, 2 * C.S + 3} <= set(C.FIELD_NEEDS)
  assert C.PAST_A_STEP == ((8193, 8192), (8193, 8193), (24581, 8193), (24581, 16384), (24581, 24580), (40000, 12000)) and C.POSITIONS_TOPK == (8192, 8193, 20000)
  assert len(C.PLACED) == 8 + 6 + 3 and all(len(C.topk_past_a_step(N, topk)) == 6 for N, topk in C.PAST_A_STEP[:1])


def test_the_key_transform_orders_as_the_definition_does():
  """``keys`` (the kernel's transform, used by the radix-depth conditions) against the stable descending sort on the special values."""
  x = torch.tensor([0.0, -0.0, 1e-45, -1e-45, 1.0, -1.0, C.INF, -C.INF, C.NAN, -C.NAN, 3e38, -3e38, 1e-39])
  k = C.keys(x)
  assert k[0] == k[1] and k[8] == k[9] == 0xFFFFFFFF and k.min() >= 0
  order = torch.sort(x, descending=True, stable=True).indices
  assert (k[order].diff() <= 0).all() and torch.equal(torch.sort(k, descending=True, stable=True).indices, order)
  assert [C.shared_bytes(a, b) for a, b in ((0x12345678, 0x12345678), (0x12345678, 0x123456FF), (0x12345678, 0x1234FF78), (0x12345678, 0x12FF5678), (0x12345678, 0x92345678))] == [4, 3, 2, 1, 0]


# ----------------------------------------------------------------------------- the sweep
def test_a_sweep_seed_is_deterministic():
  assert C.SEEDS == tuple(range(48))
  for seed in C.SEEDS:
    _identical(C.sweep_case(seed), C.sweep_case(seed))


def test_the_census_of_the_sweep():
  """Conditions on the 48 seeds, not measurements: what the sweep must reach to be worth its launches."""
  census = [C.census_of(C.sweep_case(seed)) for seed in C.SEEDS]
  families = [c["family"] for c in census if c["mode"] == "scores"]
  count = dict(scores=len(families), positions=len(census) - len(families), pass_steps=sum(c["pass_steps"] for c in census),
               tie_steps=sum(c["tie_steps"] for c in census), big_topk=sum(c["big_topk"] for c in census), **{f: families.count(f) for f in C.FAMILIES})
  print("census:", count)
  assert all(count[f] >= 1 for f in C.FAMILIES), count
  assert count["scores"] >= 1 and count["positions"] >= 1, count
  assert count["pass_steps"] >= 8 and count["tie_steps"] >= 4 and count["big_topk"] >= 4, count


def test_a_sweep_case_stays_inside_its_drawing_rules():
  for seed in C.SEEDS:
    c = C.sweep_case(seed)
    rows = c["scores"] if c["scores"] is not None else c["positions"]
    assert 1 <= rows.size(0) <= 12 and 1 <= c["topk"] <= rows.size(1) <= C.NMAX and c["page_size"] in (None, 1, 16, 48, 64), c["name"]
    assert (c["scores"] is None) != (c["positions"] is None) and rows.stride(1) == 1 and c["cache_seqlens"].numel() <= 4
    if rows.stride(0) > rows.size(1) and c["scores"] is not None:  # (what lies outside the row is NaN: the largest key there is)
      assert torch.isnan(torch.as_strided(rows, (rows.size(0), rows.stride(0)), (rows.stride(0), 1))[:, rows.size(1):]).all()


# ----------------------------------------------------------------------------- the definition against brute force, on placed rows
def _brute(row, topk):
  """Position p is selected iff fewer than topk positions beat it — hold a larger key, or an equal one at a lower position.  No sort; the keys are the kernel's
  transform, the definition uses none."""
  key = C.keys(row).numpy()
  n = key.size
  beaten = np.empty(n, dtype=np.int64)
  for lo in range(0, n, 256):
    k = key[lo: lo + 256, None]
    beaten[lo: lo + 256] = (key[None, :] > k).sum(1) + ((key[None, :] == k) & (np.arange(n)[None, :] < np.arange(lo, min(lo + 256, n))[:, None])).sum(1)
  return np.flatnonzero(beaten < topk)


@pytest.mark.parametrize("group, which, row", [("step edges", 2, 0), ("special tie values", 1, 0), ("special tie values", 1, 1)])
def test_the_definition_on_a_placed_row_is_brute_force(group, which, row):
  """Step edges at need 3, the NaN row and the -inf row at topk 9: N = 24581, the ties spread over the steps."""
  case = C.PLACED[group]()[which]
  scores, topk = case["scores"][row], case["topk"]
  want = _brute(scores, topk)
  assert want.size == topk and torch.equal(TR.select(scores, scores.numel(), topk), torch.from_numpy(want))
  idx, n = TR.topk_slots(case["scores"], topk, case["cache_seqlens"])
  assert int(n[row]) == topk and idx[row].tolist() == want.tolist()
