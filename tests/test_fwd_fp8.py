"""The FP8 forward's helper and front end without a GPU: ``quantize_attn_fp8`` (round trip, smooth-K invariance, the padded fragment layout and V8T's key
permutation restated as index arithmetic) and what ``ffpa_attn_fp8_func`` refuses, on meta tensors."""

import pytest
import torch

import model_values as mv
from ffpa_attn_amd import ffpa_attn_fp8_func, quantize_attn_fp8
from ffpa_attn_amd.interface import FP8_BLOCK_KEYS as K, FP8_BLOCK_ROWS as R

SHAPE = (2, 4, 2, R + 7, 2 * K + 19, 320)


@pytest.fixture(scope="module")
def case():
  q, k, v = mv.outliers(SHAPE, torch.bfloat16, 11)
  return q, k, v, quantize_attn_fp8(q, k, v, None, True)


def test_round_trip(case):
  q, k, v, h = case
  per_row = lambda s, blk, n: s.repeat_interleave(blk, -1)[..., :n, None]
  for x, codes, s in ((q.float() * torch.tensor(320 ** -0.5 * mv.LOG2E, dtype=torch.float32), h.q_codes, per_row(h.q_scale, R, q.size(2))),
                      (k.float() - h.k_mean[:, :, None], h.k_codes, per_row(h.k_scale, K, k.size(2))), (v.float(), h.v_codes, h.v_scale[:, :, None, :])):
    c = codes.float()
    assert bool((s == torch.exp2(torch.log2(s).round())).all()) and float(c.abs().max()) <= 448  # powers of two; no NaN code
    # half an e4m3 ulp: 2^-4 relative, 2^-10 below the normals
    assert bool(((x - c * s).abs() <= s * torch.maximum(c.abs() * 2.0 ** -4, torch.tensor(2.0 ** -10))).all())
    assert float(c.abs().amax()) > 224  # the scale is the smallest power of two that fits the block: some block uses the top binade


def test_smooth_k_leaves_the_softmax_alone(case):
  q, k, v, h = case
  ref = mv.attend(q, k, v)[0]
  smoothed = mv.attend(q, (k.double() - h.k_mean.double()[:, :, None]), v)[0]
  assert float((ref - smoothed).abs().max()) < 1e-9
  assert float(h.k_mean.abs().max()) > 0 and not bool(quantize_attn_fp8(q, k, v, None, False).k_mean.any())


@pytest.mark.parametrize("seed", range(8))
def test_layout_by_index_arithmetic(case, seed):
  q, k, v, h = case
  B, hq, hkv, nq, nkv, D = SHAPE
  dp = 384
  g = torch.Generator().manual_seed(seed)
  pick = lambda *ns: tuple(int(torch.randint(0, n, (1,), generator=g)) for n in ns)
  # q8 / k8: byte (fragment (row block, chunk) of 2 KiB, plane, lane 16 g + r, e) holds row 16 rb + r, column 128 c + 32 g + 16 plane + e; zero past N and D
  for packed, codes, blk, n in ((h.q8, h.q_codes, R, nq), (h.k8, h.k_codes, K, nkv)):
    b, hd, row, c = pick(B, codes.size(1), -(-n // blk) * blk, dp)
    frag, lane = (row % blk // 16) * (dp // 128) + c // 128, 16 * (c % 128 // 32) + row % 16
    at = frag * 2048 + (c % 32 // 16) * 1024 + 16 * lane + c % 16
    want = int(codes.view(torch.uint8)[b, hd, row, c]) if row < n and c < D else 0
    assert packed.shape[-1] == blk * dp and int(packed[b, hd, row // blk, at]) == want
  # v8t: byte (fragment db, plane, lane 16 g + r, e) holds channel 16 db + r of the tile's key 16 j + 4 g + i, j = 4 plane + e // 4, i = e % 4: accumulator
  # element i of score MFMA j in lane group g, at B position 32 g + 4 j + i
  b, hd, key, d = pick(B, hkv, -(-nkv // K) * K, D)
  j, grp, i = key % K // 16, key % 16 // 4, key % 4
  pos = 32 * grp + 4 * j + i
  at = (d // 16) * 2048 + (pos % 32 // 16) * 1024 + 16 * (16 * (pos // 32) + d % 16) + pos % 16
  want = int(h.v_codes.view(torch.uint8)[b, hd, key, d]) if key < nkv else 0
  assert h.v8t.shape[-1] == K * D and int(h.v8t[b, hd, key // K, at]) == want


REFUSALS = {
  "head dim": (dict(), 576, NotImplementedError, "head dim 576"),
  "attn_mask": (dict(attn_mask=torch.ones(8, 8, dtype=torch.bool)), 256, NotImplementedError, "attn_mask"),
  "dropout": (dict(dropout_p=0.1), 256, NotImplementedError, "dropout"),
  "lse": (dict(return_lse=True), 256, NotImplementedError, "LSE"),
  "gqa off": (dict(), 256, ValueError, "enable_gqa=False"),
}


@pytest.mark.parametrize("what", list(REFUSALS))
def test_refusals(what):
  kwargs, D, exc, word = REFUSALS[what]
  q = torch.empty(1, 4, 8, D, dtype=torch.bfloat16, device="meta")
  k = torch.empty(1, 2 if what == "gqa off" else 4, 8, D, dtype=torch.bfloat16, device="meta")
  with pytest.raises(exc, match=word):
    ffpa_attn_fp8_func(q, k, k, **kwargs)


def test_inference_only_and_gpu_only():
  q = torch.zeros(1, 1, 8, 256, dtype=torch.bfloat16)
  with pytest.raises(NotImplementedError, match="is inference only: query requires grad and there is no backward"):
    ffpa_attn_fp8_func(q.clone().requires_grad_(), q, q)
  with pytest.raises(NotImplementedError, match="no implementation for device 'cpu'"):
    ffpa_attn_fp8_func(q, q, q)


def test_the_stated_tile_is_the_librarys():
  from ffpa_attn_amd import hip

  for D in hip.FP8_HEAD_DIMS:  # (no device needed: the query only formats the kernel's name, and fp8_forward_kernel raises where the constants differ)
    assert f"ffpa_fwd_fp8_kernel<{D}, fp16> rows={R} keys={K} " in hip.fp8_forward_kernel(D, fp16=True)
