"""What tests/test_kvcache_mla_contract_gpu.py draws on the CPU, checked without a GPU: the chunk counts of its row shapes against ``hip.mla_row_chunks``, and
the property every model-like case must show on its float64 reference before it is worth a launch."""

import pytest
import torch

import kvcache_mla_cases as C
import kvcache_ref as R
from ffpa_attn_amd import hip


@pytest.mark.parametrize("hq, hkv, sq", C.ROW_SHAPES)
def test_row_shapes_have_the_chunk_counts_the_gpu_module_asserts(hq, hkv, sq):
  group = hq // hkv
  chunks = hip.mla_row_chunks(group, sq)
  assert len(chunks) == C.row_tiles(hq, hkv, sq)
  assert all(len(c) == C.BLOCK_ROWS for c in chunks[:-1]) and len(chunks[-1]) == C.live_rows_of_last_chunk(hq, hkv, sq)
  assert len(chunks[-1]) < C.BLOCK_ROWS, "every row shape of the module ends in a partial chunk"
  assert [r for c in chunks for r in c] == [(h, t) for h in range(group) for t in range(sq)]  # head-major, every row once
  if C.packed(hq, hkv):
    assert len(chunks) > 1 and C.row_tiles(hq, hkv, sq) == -(-group * sq // 64)
  else:
    assert C.row_tiles(hq, hkv, sq) == -(-sq // 64) and len(chunks) > 1


def test_the_boundaries_the_issue_names():
  assert hip.mla_row_chunks(32, 3)[1][0] == (21, 1) and len(hip.mla_row_chunks(32, 3)[1]) == 32
  assert [len(c) for c in hip.mla_row_chunks(24, 3)] == [64, 8]
  assert [len(c) for c in hip.mla_row_chunks(40, 5)] == [64, 64, 64, 8]
  chunks = hip.mla_row_chunks(16, 70)
  assert len(chunks) == 18 and len(chunks[-1]) == 32
  assert all(1 <= len({h for h, _ in c}) <= 2 for c in chunks)  # Sq > 64: a chunk holds part of one or two heads' tokens
  assert any(len({h for h, _ in c}) == 1 and len(c) == 64 for c in chunks)
  for sq in (3, 5, 70, 130):
    assert {0, sq - 1, sq, sq + 1} <= set(C.row_lens(sq))


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("variant", C.MODEL_VARIANTS)
def test_every_model_like_case_shows_its_familys_property(variant, dtype):
  cases = C.model_cases(variant, R.TORCH_DTYPE[dtype])
  assert len(cases) == len(C.MODEL_HEADS) * len(C.MODEL_SQ) * len(C.MODEL_LENS)
  for case in cases:
    q, k = C.build_model_case(case)
    B, hq, hkv, sq, L, d = case["shape"]
    assert q.shape == (B, hq, sq, d) and k.shape == (B, hkv, L, d) and d == C.D
    ref = C.model_reference(case, q, k)
    assert ref[0].shape == (B, sq, hq, C.DV) and bool(torch.isfinite(ref[1]).all())  # (key 0 is in every row's view)
    C.assert_family_property(case, q, k, ref)
