"""Tree-mask attention without a GPU: the float64 restatement (tests/tree_ref.py) against a per-row brute-force loop and against ``kvcache_ref.attend`` at the
two masks the plain call can express, the bit layout of ``pack_tree_mask``, every host-side refusal of ``ffpa_attn_with_kvcache_tree`` (on meta / CPU tensors,
before any device work), the fake op, and the draw of the GPU sweep (tests/test_tree_gpu.py)."""

import random

import pytest
import torch

import kvcache_ref as R
import tree_ref as T
from ffpa_attn_amd import ffpa_attn_with_kvcache_tree, pack_tree_mask


def _problem(seed, B=3, sq=5, heads=(4, 2), d=16, page=64, lens=(66, 5, 3)):
  g = torch.Generator().manual_seed(seed)
  hq, hkv = heads
  q = torch.randn((B, sq, hq, d), generator=g, dtype=torch.float64)
  if page:
    pps = -(-max(lens) // page) + 1
    n_pages = B * pps + 2
    kc, vc = torch.randn((n_pages, page, hkv, d), generator=g, dtype=torch.float64), torch.randn((n_pages, page, hkv, d), generator=g, dtype=torch.float64)
    table = torch.randperm(n_pages, generator=g)[: B * pps].to(torch.int32).view(B, pps)
  else:
    cap = max(lens) + 7
    kc, vc = torch.randn((B, cap, hkv, d), generator=g, dtype=torch.float64), torch.randn((B, cap, hkv, d), generator=g, dtype=torch.float64)
    table = None
  return q, kc, vc, list(lens), table


@pytest.mark.parametrize("page", [64, 0])
@pytest.mark.parametrize("kind", T.MASK_KINDS)
@pytest.mark.parametrize("per_sequence", [False, True])
def test_reference_equals_a_per_row_brute_force_loop(page, kind, per_sequence):
  """Lengths 66 / 5 / 3 / 0 at Sq 5: draft keys behind a prefix, L == Sq, L < Sq (draft positions below 0 do not exist), no key at all."""
  lens = (66, 5, 3, 0)
  q, kc, vc, lens, table = _problem(11, B=4, lens=lens, page=page)
  rng = random.Random(3)
  mask = torch.stack([T.draw_mask(kind, 5, rng) for _ in range(4)]) if per_sequence else T.draw_mask(kind, 5, rng)
  o, lse, pmax, p2sum = T.attend_tree(q, kc, vc, lens, table, mask)
  o_b, lse_b = T.brute_force(q, kc, vc, lens, table, mask)
  assert torch.equal(torch.isneginf(lse), torch.isneginf(lse_b))
  fin = torch.isfinite(lse_b)
  torch.testing.assert_close(o, o_b, atol=1e-12, rtol=1e-12)
  torch.testing.assert_close(lse[fin], lse_b[fin], atol=1e-12, rtol=1e-12)
  assert (o[3] == 0).all() and torch.isneginf(lse[3]).all()  # the empty sequence
  assert ((pmax >= 0) & (pmax <= 1)).all() and (p2sum <= pmax + 1e-12).all()
  if kind == "random" and not per_sequence:  # the all-False row sees the prefix only: at L <= Sq there is none
    dead = (~mask.any(dim=1)).nonzero().flatten().tolist()
    assert dead and all(torch.isneginf(lse[1, :, i]).all() and (o[1, i] == 0).all() for i in dead)


@pytest.mark.parametrize("page", [64, 0])
def test_tril_is_the_causal_call_and_ones_the_plain_call_exactly(page):
  q, kc, vc, lens, table = _problem(5, B=4, sq=6, lens=(130, 6, 4, 0), page=page)
  for mask, causal in ((torch.tril(torch.ones((6, 6), dtype=torch.bool)), True), (torch.ones((6, 6), dtype=torch.bool), False)):
    got = T.attend_tree(q, kc, vc, lens, table, mask)
    want = R.attend(q, kc, vc, lens, table, causal)
    for g, w in zip(got, want):
      assert torch.equal(g, w)
    got_b = T.attend_tree(q, kc, vc, lens, table, mask[None].expand(4, 6, 6))
    for g, w in zip(got_b, want):
      assert torch.equal(g, w)


def test_tree_masks_from_parent_arrays():
  m = T.tree_mask_from_parents([-1, 0, 0, 1, 3, 2])
  want = torch.tensor([[1, 0, 0, 0, 0, 0], [1, 1, 0, 0, 0, 0], [1, 0, 1, 0, 0, 0], [1, 1, 0, 1, 0, 0], [1, 1, 0, 1, 1, 0], [1, 0, 1, 0, 0, 1]], dtype=torch.bool)
  assert torch.equal(m, want)


# ----------------------------------------------------------------------------- pack_tree_mask
def test_pack_tree_mask_bit_layout():
  m = torch.zeros((64, 64), dtype=torch.bool)
  m[0, 0] = m[1, 63] = m[2, 5] = m[2, 40] = True
  m[3] = True
  w = pack_tree_mask(m)
  assert w.dtype == torch.int64 and tuple(w.shape) == (1, 64)
  assert w[0, 0].item() == 1
  assert w[0, 1].item() == -(2 ** 63)  # bit 63: the sign bit
  assert w[0, 2].item() == (1 << 5) | (1 << 40)
  assert w[0, 3].item() == -1
  assert (w[0, 4:] == 0).all()
  # every bit, against Python integers; the shared [Sq, Sq] form is row 0 of the batched one
  rng = random.Random(1)
  for sq in (1, 2, 31, 32, 33, 63, 64):
    mb = torch.tensor([[[rng.random() < 0.5 for _ in range(sq)] for _ in range(sq)] for _ in range(3)], dtype=torch.bool).reshape(3, sq, sq)
    wb = pack_tree_mask(mb)
    assert tuple(wb.shape) == (3, sq)
    for b in range(3):
      for i in range(sq):
        want = sum(1 << j for j in range(sq) if mb[b, i, j])
        assert wb[b, i].item() & (2 ** 64 - 1) == want
    assert torch.equal(pack_tree_mask(mb[1]), wb[1:2])
  assert pack_tree_mask(torch.ones((2, 2), dtype=torch.bool, device="meta")).shape == (1, 2)


@pytest.mark.parametrize("mask, exc, text", [
  ([[True]], TypeError, "must be a tensor"),
  (torch.ones((4, 4), dtype=torch.uint8), TypeError, "torch.bool"),
  (torch.ones((4,), dtype=torch.bool), ValueError, r"\[Sq, Sq\] or \[B, Sq, Sq\]"),
  (torch.ones((4, 5), dtype=torch.bool), ValueError, r"\[Sq, Sq\] or \[B, Sq, Sq\]"),
  (torch.ones((2, 2, 4, 4), dtype=torch.bool), ValueError, r"\[Sq, Sq\] or \[B, Sq, Sq\]"),
  (torch.ones((65, 65), dtype=torch.bool), ValueError, r"outside \[1, 64\]"),
  (torch.ones((0, 0), dtype=torch.bool), ValueError, r"outside \[1, 64\]"),
])
def test_pack_tree_mask_refusals(mask, exc, text):
  with pytest.raises(exc, match=text):
    pack_tree_mask(mask)


# ----------------------------------------------------------------------------- the public call: everything it refuses, it refuses before touching a device
def _meta(*shape, dtype=torch.bfloat16):
  return torch.empty(*shape, dtype=dtype, device="meta")


def _call(**over):
  args = dict(q=_meta(2, 4, 32, 128), k_cache=_meta(2, 256, 8, 128), v_cache=_meta(2, 256, 8, 128), cache_seqlens=_meta(2, dtype=torch.int32),
              tree_mask=_meta(4, 4, dtype=torch.bool))
  args.update(over)
  return ffpa_attn_with_kvcache_tree(**args)


@pytest.mark.parametrize("kw, exc, text", [
  (dict(tree_mask=None), TypeError, "tree_mask must be a tensor"),
  (dict(tree_mask=[[True] * 4] * 4), TypeError, "tree_mask must be a tensor"),
  (dict(tree_mask=_meta(4, 4, dtype=torch.uint8)), TypeError, "tree_mask must be a torch.bool mask or int64"),
  (dict(tree_mask=_meta(4, 4, dtype=torch.int32)), TypeError, "tree_mask must be a torch.bool mask or int64"),
  (dict(tree_mask=_meta(4, 4, dtype=torch.float32)), TypeError, "tree_mask must be a torch.bool mask or int64"),
  (dict(tree_mask=_meta(4, dtype=torch.bool)), ValueError, "tree_mask must be bool"),
  (dict(tree_mask=_meta(4, 5, dtype=torch.bool)), ValueError, "tree_mask must be bool"),
  (dict(tree_mask=_meta(5, 5, dtype=torch.bool)), ValueError, "tree_mask must be bool"),
  (dict(tree_mask=_meta(3, 4, 4, dtype=torch.bool)), ValueError, "tree_mask must be bool"),
  (dict(tree_mask=_meta(1, 2, 4, 4, dtype=torch.bool)), ValueError, "tree_mask must be bool"),
  (dict(tree_mask=_meta(3, 4, dtype=torch.int64)), ValueError, "packed tree_mask must be int64"),
  (dict(tree_mask=_meta(2, 5, dtype=torch.int64)), ValueError, "packed tree_mask must be int64"),
  (dict(tree_mask=_meta(2, 4, 1, dtype=torch.int64)), ValueError, "packed tree_mask must be int64"),
  (dict(tree_mask=torch.ones((4, 4), dtype=torch.bool)), ValueError, "tree_mask must be on q's device"),
  (dict(q=_meta(2, 65, 32, 128), tree_mask=_meta(65, 65, dtype=torch.bool)), ValueError, r"tree_mask needs 1 <= Sq <= 64"),
  (dict(q=_meta(2, 0, 32, 128), tree_mask=_meta(0, 0, dtype=torch.bool)), ValueError, r"tree_mask needs 1 <= Sq <= 64"),
  # ffpa_attn_with_kvcache's own checks, through the shared validation
  (dict(q=_meta(2, 4, 32, 128, dtype=torch.float32)), TypeError, "fp16/bf16"),
  (dict(q=_meta(2, 4, 30, 128)), ValueError, "num_heads"),
  (dict(k_cache=_meta(3, 256, 8, 128), v_cache=_meta(3, 256, 8, 128)), ValueError, "q's batch"),
  (dict(num_splits=-1), ValueError, "num_splits"),
  (dict(cache_seqlens=_meta(3, dtype=torch.int32)), ValueError, "cache_seqlens"),
  (dict(k=_meta(2, 4, 8, 128), v=_meta(2, 3, 8, 128)), ValueError, "share their shape"),
  (dict(k=_meta(2, 4, 8, 128), v=_meta(2, 4, 8, 128), cache_seqlens=None), ValueError, "cache_seqlens is required"),
  (dict(k=_meta(2, 4, 8, 128)), NotImplementedError, "does not support: k"),
  (dict(block_table=_meta(2, 4, dtype=torch.int32), k_cache=_meta(16, 48, 8, 128), v_cache=_meta(16, 48, 8, 128)), ValueError, "page_size"),
])
def test_host_checks_of_the_tree_call(kw, exc, text):
  with pytest.raises(exc, match=text):
    _call(**kw)


def test_the_tree_call_has_no_rotary_parameters_and_is_inference_only():
  with pytest.raises(TypeError, match="rotary_cos"):
    _call(rotary_cos=_meta(256, 32), rotary_sin=_meta(256, 32))
  with pytest.raises(TypeError, match="tree_mask"):  # keyword-only and required
    ffpa_attn_with_kvcache_tree(_meta(2, 4, 32, 128), _meta(2, 256, 8, 128), _meta(2, 256, 8, 128))
  for name in ("q", "k_cache", "v_cache"):
    t = torch.zeros((2, 256, 8, 128) if name != "q" else (2, 4, 32, 128), dtype=torch.bfloat16, requires_grad=True)
    kw = dict(q=torch.zeros((2, 4, 32, 128), dtype=torch.bfloat16), k_cache=torch.zeros((2, 256, 8, 128), dtype=torch.bfloat16),
              v_cache=torch.zeros((2, 256, 8, 128), dtype=torch.bfloat16), cache_seqlens=torch.zeros(2, dtype=torch.int32),
              tree_mask=torch.ones((4, 4), dtype=torch.bool))
    kw[name] = t
    with pytest.raises(NotImplementedError, match=f"is inference only: {name} requires grad and there is no backward"):
      ffpa_attn_with_kvcache_tree(**kw)
  # CPU tensors that pass every check reach the op, which has no CPU kernel: an error, never a fall-back
  kw[name] = kw[name].detach()
  with pytest.raises(NotImplementedError):
    ffpa_attn_with_kvcache_tree(**kw)


@pytest.mark.parametrize("paged", [False, True])
@pytest.mark.parametrize("form", ["shared", "batched", "packed"])
def test_fake_op_and_public_call_shapes_on_meta(paged, form):
  q = _meta(3, 7, 32, 512)
  kc = _meta(40, 128, 8, 512) if paged else _meta(3, 640, 8, 512)
  bt = _meta(3, 5, dtype=torch.int32) if paged else None
  mask = {"shared": _meta(7, 7, dtype=torch.bool), "batched": _meta(3, 7, 7, dtype=torch.bool), "packed": _meta(3, 7, dtype=torch.int64)}[form]
  for kv in (None, _meta(3, 7, 8, 512)):
    out, lse = ffpa_attn_with_kvcache_tree(q, kc, kc, kv, kv, cache_seqlens=_meta(3, dtype=torch.int32), block_table=bt, tree_mask=mask, return_softmax_lse=True)
    assert tuple(out.shape) == (3, 7, 32, 512) and out.dtype == torch.bfloat16
    assert tuple(lse.shape) == (3, 32, 7) and lse.dtype == torch.float32
  out = ffpa_attn_with_kvcache_tree(q, kc, kc, cache_seqlens=5, block_table=bt, tree_mask=mask)
  assert tuple(out.shape) == (3, 7, 32, 512)


# ----------------------------------------------------------------------------- the GPU sweep's draw
def test_the_sweep_covers_its_axes_and_at_most_a_quarter_of_its_rows_see_no_key():
  cases = [T.draw_case(s) for s in T.SWEEP_SEEDS]
  assert len(cases) == 40
  seen = total = 0
  for c in cases:
    assert 1 <= c["Sq"] <= 64 and 0 <= min(c["lens"]) and max(c["lens"]) <= 5000
    s, t = T.visible_rows(c)
    seen, total = seen + s * c["heads"][0], total + t * c["heads"][0]
  assert total - seen <= total // 4, (seen, total)
  assert {c["page"] for c in cases} == {64, 128, 0}
  assert {c["dtype"] for c in cases} == {"bf16", "fp16"}
  assert {c["num_splits"] for c in cases} == {0, 1, 3}
  assert {c["mask_kind"] for c in cases} == set(T.MASK_KINDS)
  assert {c["per_sequence"] for c in cases} == {False, True}
  assert {c["head_dim_class"] for c in cases} == set(R.PAGED_HEAD_DIM_CLASSES)
  assert {1, 64} <= {c["Sq"] for c in cases}
  assert any(max(c["lens"]) > 2500 for c in cases) and any(0 in c["lens"] for c in cases)
  assert any(c["heads"][0] == c["heads"][1] for c in cases) and any(c["heads"][0] != c["heads"][1] for c in cases)
