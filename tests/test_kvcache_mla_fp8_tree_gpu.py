"""``ffpa_attn_with_kvcache_mla_tree_fp8`` / ``ffpa_attn_varlen_with_kvcache_mla_tree_fp8`` on the GPU: the latent kernel's tree build over a cache of OCP e4m3 codes
(``ffpa_fwd_m16_mla_tree_fp8_kernel``: the MLA, the tree and the FP8 hook of the tile text on) and the quantising appends in front of it.

Two references.  (1) NO TOLERANCE: with a power-of-two ``kv_scale`` the call returns the bits of ``ffpa_attn_with_kvcache_mla_tree`` on ``pool8.to(dtype)`` under
``softmax_scale * kv_scale``, O scaled by ``kv_scale`` — the LSE in both dtypes and bf16 O (fp16 O is held by (2) only: DESIGN section 15).  (2) float64 tree
attention (tests/tree_ref.py ``attend_tree``, the 16-bit tree suite's construction) on ``pool8.double() * kv_scale`` with ``kv_scale = 0.37``, outputs held to
``kvcache_ref.check`` / ``allowance`` unchanged, LSE to atol 2e-4 / rtol 2e-5 — no new tolerance, as in tests/test_kvcache_mla_fp8_gpu.py.  The appends are held to
``quantize_latent_rows`` byte for byte (NaN codes by NaN-ness).

D = 576, head_dim_v = 512, scale 1 / sqrt(192), pages of 64 keys shuffled in a pool that holds the FP8 NaN code in every byte no sequence owns (the cases are
tests/test_kvcache_mla_fp8_gpu.py's).  The key lengths are the 16-bit tree suite's ``_lens(sq)`` and a sequence of ONE key more: its only row holds zero codes, so
the tokens that see it see nothing else; row 0 and the last row of the 300-key sequence hold +-448 codes — the first is in every token's prefix."""

import contextlib

import numpy as np
import pytest
import torch

import kvcache_ref as R
import tree_ref as T
from test_fwd_gpu import hip  # noqa: F401  (fixture)
from test_kvcache_mla_fp8_gpu import NAN8, _case, _pool_of, _same_bits, _same_codes, _same_out, _write_rows
from test_kvcache_mla_tree_gpu import RAGGED, _lens, _mask

pytestmark = pytest.mark.gpu

D, DV, PAGE = 576, 512, 64
SCALE = 192 ** -0.5
HEADS = [(1, 1), (16, 1), (128, 1), (32, 2)]
TOKENS = [1, 2, 5, 33, 64]
F8 = torch.float8_e4m3fn
KERNEL = "ffpa_fwd_m16_mla_tree_fp8_kernel"
TWIN = "ffpa_fwd_m16_mla_tree_kernel"


@contextlib.contextmanager
def _launches(hip, flags=0, record=True):
  """Every latent launch inside the block — every latent call goes through ``hip.mla_forward`` — carries ``flags`` too, and (``record``) its plan is appended to the
  list the block receives."""
  plans, real = [], hip.mla_forward

  def spy(*args, **kw):
    kw["flags"] = kw.get("flags", 0) | flags
    if not record:
      return real(*args, **kw)
    plan = {}
    kw["plan_out"] = plan
    out = real(*args, **kw)
    plans.append(plan)
    return out

  hip.mla_forward = spy
  try:
    yield plans
  finally:
    hip.mla_forward = real


def _the_new_kernel_and_no_other(plans, dtype, n=1):
  assert len(plans) == n and all(p["kernel"].startswith(f"{KERNEL}<{dtype}, 576, dv=512") for p in plans), plans


_TCASES: dict = {}


def _tcase(sq, hq, hkv, dtype, lens=None, **kw):
  """The FP8 latent suite's case (shared, never written) for ``_lens(sq)`` plus a sequence of one key, on a storage of its own in which the FIRST row of the
  longest sequence holds +-448 codes as well: a prefix row, visible to every token of that sequence under any mask."""
  lens = sorted(set(_lens(sq)) | {1}) if lens is None else lens
  key = (sq, hq, hkv, dtype, tuple(lens), tuple(sorted(kw.items())))
  if key in _TCASES:
    return _TCASES[key]
  base = _case(lens, hq, hkv, sq, dtype, seed=hq + sq, **kw)
  storage = base["storage"].clone()
  view = R.reviewed(base["view"], base["storage"], storage)
  longest = max(range(len(lens)), key=lambda b: lens[b])
  if lens[longest] > sq + 1:
    slab = (longest, 0) if base["ids"] is None else (int(base["ids"][longest, 0]), 0)
    view[slab] = torch.tensor([0xFE, 0x7E], dtype=torch.uint8, device="cuda").repeat(D // 2)
  t = dict(base, storage=storage, view=view, pool=view.view(F8), refs={}, extra=[b for b, n in enumerate(lens) if n == 1 and 1 not in _lens(sq)])
  _TCASES[key] = t
  return t


def _tree8(hip, t, mask, *, kv_scale=1.0, num_splits=0, flags=0, lens=None, kv=None, pool=None, q=None, table="case"):
  from ffpa_attn_amd import ffpa_attn_with_kvcache_mla_tree_fp8

  with _launches(hip, flags) as plans:
    out, lse = ffpa_attn_with_kvcache_mla_tree_fp8(t["q"] if q is None else q, t["pool"] if pool is None else pool, DV, kv_scale=kv_scale, tree_mask=mask.cuda(), kv=kv,
                                                   cache_seqlens=t["lens"] if lens is None else lens, block_table=t["table"] if isinstance(table, str) else table,
                                                   softmax_scale=SCALE, num_splits=num_splits, return_softmax_lse=True)
  _the_new_kernel_and_no_other(plans, t["dtype"])
  return out, lse, plans[0]


def _wide(hip, t, mask, kv_scale, *, num_splits=0, flags=0):
  """The 16-bit tree call on the dequantised pool: ``pool8.to(dtype)`` under ``softmax_scale * kv_scale``, O scaled by ``kv_scale``."""
  from ffpa_attn_amd import ffpa_attn_with_kvcache_mla_tree

  pool16 = t["pool"].to(R.TORCH_DTYPE[t["dtype"]]).contiguous()
  with _launches(hip, flags) as plans:
    out, lse = ffpa_attn_with_kvcache_mla_tree(t["q"], pool16, DV, tree_mask=mask.cuda(), cache_seqlens=t["lens"], block_table=t["table"], softmax_scale=SCALE * kv_scale,
                                               num_splits=num_splits, return_softmax_lse=True)
  assert len(plans) == 1 and plans[0]["kernel"].startswith(f"{TWIN}<{t['dtype']}, 576, dv=512"), plans
  return out * kv_scale, lse, plans[0]


def _ref(t, mask, kv_scale, lens=None, pool=None, q=None, table="case", guard=True):
  """The tree suite's reference on the dequantised pool: float64 tree attention on (deq, deq), value columns ``[:512]``, with that suite's two conditions asserted
  on it — no NaN, and at least three quarters of the query rows of the ``_lens`` sequences see a key — -> (reference tuple, vstat of the visible values)."""
  pool = t["pool"] if pool is None else pool
  q = t["q"] if q is None else q
  lens = t["lens_list"] if lens is None else lens
  table = t["table"] if isinstance(table, str) else table
  deq = pool.double() * kv_scale
  o, lse, pmax, p2sum = T.attend_tree(q, deq, deq, lens, table, mask, SCALE)
  ref = (o[..., :DV].contiguous(), lse, pmax, p2sum)
  assert not any(bool(torch.isnan(x).any()) for x in ref), "the reference holds NaN"
  if guard:
    sq, cap = q.size(1), R.capacity_of(pool, table)
    own = [b for b in range(len(lens)) if b not in t.get("extra", [])]
    seen = sum(int(T.visible(mask, b, min(max(int(lens[b]), 0), cap), sq).any(dim=1).sum()) for b in own if min(max(int(lens[b]), 0), cap) > 0)
    assert 4 * seen >= 3 * len(own) * sq, f"only {seen} of {len(own) * sq} query rows see a key: the case could hide a failure behind empty rows"
  return ref, R.visible_values(deq[..., :DV], lens, table)


def _hold(out, lse, ref, vstat, dtype, name):
  ratio = R.check(out, lse, ref, v=vstat, dtype=dtype, name=name)
  empty = torch.isneginf(ref[1]).permute(0, 2, 1)  # [B, Sq, Hq]: rows that see nothing, exactly
  assert (out[empty] == 0).all() and torch.isneginf(lse.permute(0, 2, 1)[empty]).all(), name
  print(f"[mla tree fp8] {ratio:.3f} {name}")
  return ratio


def _case_mask(kind, sq, hq, lens):
  """The 16-bit tree suite's mask of the case (per-sequence and shared masks alternate over the cases) — with the one-key sequence's own mask, where no token of it
  would see its key, given the last token's diagonal bit: the batch then holds a token whose ONLY key is that sequence's row."""
  B, b1 = len(lens), lens.index(1)
  per_sequence = (hq + sq + len(kind)) % 2 == 0
  mask = _mask(kind, sq, B, per_sequence, seed=sq + hq)
  if not bool(T.visible(mask, b1, 1, sq).any()):
    mask = (mask if mask.dim() == 3 else mask[None].expand(B, sq, sq)).clone()
    mask[b1, sq - 1, sq - 1] = True
    per_sequence = True
  assert bool(T.visible(mask, b1, 1, sq).any())
  return mask, per_sequence


CASES = [(hq, hkv, sq) for hq, hkv in HEADS for sq in TOKENS]


# ----------------------------------------------------------------------------- 1. bit identity with the 16-bit tree kernel on the dequantised pool
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("hq, hkv, sq", CASES)
@pytest.mark.parametrize("kind", ["tree", "random", "sparse"])
def test_power_of_two_scales_return_the_bits_of_the_16_bit_tree_call(hip, dtype, hq, hkv, sq, kind):
  """kv_scale 1, 0.25 and 8; the same forced KV ranges (1, 2, 3, 5: ranges start at odd tiles, some are empty) and the same non-temporal choice on both arms.  The
  image the FP8 build writes is the image the LDS-DMA writes, the mask words meet the same scores: LSE (both dtypes) and bf16 O are the 16-bit call's bits, and the
  plan names the new kernel with the twin's workgroups and splits."""
  t = _tcase(sq, hq, hkv, dtype)
  B = len(t["lens_list"])
  mask, per_sequence = _case_mask(kind, sq, hq, t["lens_list"])
  runs = [(1.0, 1, hip.FLAG_NO_KV_STREAM), (1.0, 2, hip.FLAG_KV_STREAM), (0.25, 3, hip.FLAG_NO_KV_STREAM), (0.25, 1, hip.FLAG_KV_STREAM), (8.0, 5, hip.FLAG_KV_STREAM),
          (8.0, 2, hip.FLAG_NO_KV_STREAM)]
  for kv_scale, ns, stream in runs:
    flags = hip.FLAG_FORCE_SPLITS | stream
    out, lse, plan = _tree8(hip, t, mask, kv_scale=kv_scale, num_splits=ns, flags=flags)
    want, want_lse, want_plan = _wide(hip, t, mask, kv_scale, num_splits=ns, flags=flags)
    what = f"{dtype} heads {(hq, hkv)} Sq {sq} {kind} kv_scale {kv_scale} splits {ns} -> {plan}"
    assert plan["splits"] == ns == want_plan["splits"] and (", NT>" in plan["kernel"]) == (stream == hip.FLAG_KV_STREAM) == (", NT>" in want_plan["kernel"]), what
    assert plan["kernel"] == want_plan["kernel"].replace("_mla_tree_kernel", "_mla_tree_fp8_kernel") and plan["workgroups"] == want_plan["workgroups"], what
    assert plan["row_tiles"] == want_plan["row_tiles"] and plan["block_keys"] == 32 and plan.get("compact_slots") == want_plan.get("compact_slots"), what
    assert out.shape == (B, sq, hq, DV) and (out[0] == 0).all() and torch.isneginf(lse[0]).all()  # (L = 0)
    assert not torch.isnan(out).any() and not torch.isnan(lse).any(), what  # (no NaN byte was read)
    assert _same_bits(lse, want_lse), f"LSE: {what}: {int((lse != want_lse).sum())} rows differ"
    if dtype == "bf16":
      assert _same_bits(out, want), f"O: {what}: {int((out != want).sum())} elements differ, max {(out.float() - want.float()).abs().max().item():.3e}"


# ----------------------------------------------------------------------------- 2. against float64
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("hq, hkv, sq", CASES)
@pytest.mark.parametrize("kind", ["tree", "random", "sparse"])
def test_a_scale_that_is_no_power_of_two_against_float64(hip, dtype, hq, hkv, sq, kind):
  """kv_scale = 0.37 on the same cases, with the library's own split count and with three forced ranges.  The batch holds rows of +-448 codes (one in the prefix
  of the 300-key sequence: visible to all of its tokens) and a sequence whose only key is a row of zero codes: the tokens that see it return O = 0, LSE = 0."""
  t = _tcase(sq, hq, hkv, dtype)
  lens = t["lens_list"]
  B = len(lens)
  mask, per_sequence = _case_mask(kind, sq, hq, lens)
  b300, b1 = lens.index(300), lens.index(1)
  assert ((t["view"][int(t["ids"][b300, 0]), 0] & 0x7F) == 0x7E).all() and (t["view"][int(t["ids"][b1, 0]), 0] == 0).all()
  ref, vstat = _ref(t, mask, 0.37)
  assert vstat[0] == pytest.approx(448 * 0.37)
  for kw in ({}, dict(num_splits=3, flags=hip.FLAG_FORCE_SPLITS)):
    out, lse, plan = _tree8(hip, t, mask, kv_scale=0.37, **kw)
    name = f"float64: {dtype} heads {(hq, hkv)} Sq {sq} {kind} {'per sequence' if per_sequence else 'shared'} {kw} -> {plan}"
    _hold(out, lse, ref, vstat, dtype, name)
    sees = T.visible(mask, b1, 1, sq).any(dim=1).cuda()  # [Sq]: the tokens of the one-key sequence that see its key — a row of zeros: p = 1 on it, LSE = 0
    assert bool(sees.any()) and (out[b1] == 0).all()
    assert lse[b1][:, sees].abs().max().item() <= R.LSE_ATOL and torch.isneginf(lse[b1][:, ~sees]).all()


# ----------------------------------------------------------------------------- 3. identities
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("hq, hkv, sq", [(16, 1, 1), (16, 1, 3), (16, 1, 5), (128, 1, 3), (32, 2, 33), (1, 1, 5), (16, 1, 64)])
def test_tril_is_the_causal_fp8_latent_call_and_all_ones_the_plain_one(hip, dtype, hq, hkv, sq):
  from ffpa_attn_amd import ffpa_attn_with_kvcache_mla_fp8, pack_tree_mask

  t = _tcase(sq, hq, hkv, dtype)
  for causal, mask in ((True, torch.ones(sq, sq, dtype=torch.bool).tril()), (False, torch.ones(sq, sq, dtype=torch.bool))):
    for ns in (1, 3):
      flags = hip.FLAG_FORCE_SPLITS if ns > 1 else 0
      got = _tree8(hip, t, mask, kv_scale=0.37, num_splits=ns, flags=flags)
      with _launches(hip, flags) as plans:
        want = ffpa_attn_with_kvcache_mla_fp8(t["q"], t["pool"], DV, kv_scale=0.37, cache_seqlens=t["lens"], block_table=t["table"], softmax_scale=SCALE, causal=causal,
                                              num_splits=ns, return_softmax_lse=True)
      assert len(plans) == 1 and plans[0]["kernel"].startswith("ffpa_fwd_m16_mla_fp8_kernel") and plans[0]["splits"] == got[2]["splits"] == ns, plans
      assert _same_bits(got[1], want[1]), f"causal={causal} ranges {ns}: LSE differs"
      if dtype == "bf16":
        assert _same_bits(got[0], want[0]), f"causal={causal} ranges {ns}: {int((got[0] != want[0]).sum())} elements differ"
      else:
        assert ((got[0].double() - want[0].double()).abs() <= R.ulp_of(want[0].double(), dtype)).all()
    again = _tree8(hip, t, pack_tree_mask(mask.cuda()), kv_scale=0.37, num_splits=1)  # (packed words: the same launch)
    first = _tree8(hip, t, mask, kv_scale=0.37, num_splits=1)
    assert _same_bits(again[0], first[0]) and _same_bits(again[1], first[1])


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("hq, hkv, sq", [(16, 1, 2), (16, 1, 5), (1, 1, 5), (128, 1, 33)])
def test_the_nt_build_is_bit_identical_to_the_plain_build(hip, dtype, hq, hkv, sq):
  t = _tcase(sq, hq, hkv, dtype)
  mask = _mask("tree", sq, len(t["lens_list"]), False, seed=sq)
  for ns in (1, 3):
    force = hip.FLAG_FORCE_SPLITS if ns > 1 else 0
    plain = _tree8(hip, t, mask, kv_scale=0.37, num_splits=ns, flags=force | hip.FLAG_NO_KV_STREAM)
    nt = _tree8(hip, t, mask, kv_scale=0.37, num_splits=ns, flags=force | hip.FLAG_KV_STREAM)
    assert ", NT>" in nt[2]["kernel"] and ", NT>" not in plain[2]["kernel"], (plain[2], nt[2])
    assert _same_bits(plain[0], nt[0]) and _same_bits(plain[1], nt[1])
  ref, vstat = _ref(t, mask, 0.37)
  _hold(nt[0], nt[1], ref, vstat, dtype, f"NT build {dtype} heads {(hq, hkv)} Sq {sq}")


# ----------------------------------------------------------------------------- 4. ragged batches
def _ragged_case(qlens, cache, hq, hkv, dtype, seed, pad=2, room=8):
  """A ragged step over an FP8 pool: q and the new rows ``kv`` (``pad`` rows of NaN behind the batch's last token), the pool (a view of a uint8 storage with a page
  of the NaN code on either side; the NaN code in every row no sequence holds), the shuffled block table and the lengths BEFORE the step."""
  from ffpa_attn_amd import quantize_latent_rows

  g = torch.Generator(device="cuda").manual_seed(5000 + seed)
  tdt = R.TORCH_DTYPE[dtype]
  B, Tq = len(qlens), sum(qlens)
  q = torch.randn((Tq + pad, hq, D), generator=g, device="cuda", dtype=tdt)
  kv = torch.randn((Tq + pad, hkv, D), generator=g, device="cuda", dtype=torch.float32).mul_(2).to(tdt)
  kv[Tq:] = float("nan")
  pps = -(-(max(h + n for h, n in zip(cache, qlens)) + room + 1) // PAGE)
  n_pages = B * pps + 3
  ids = torch.randperm(n_pages, generator=torch.Generator().manual_seed(seed))[: B * pps].to(torch.int32).view(B, pps)
  codes = quantize_latent_rows(torch.randn((n_pages, PAGE, hkv, D), generator=g, device="cuda"), 1.0).view(torch.uint8)
  seen = torch.zeros((n_pages, PAGE), dtype=torch.bool)
  for b, n in enumerate(cache):
    for j in range(n):
      seen[int(ids[b, j // PAGE]), j % PAGE] = True
  codes[~seen.cuda()] = NAN8
  storage = torch.full((n_pages + 2, PAGE, hkv, D), NAN8, dtype=torch.uint8, device="cuda")
  view = storage[1:-1]
  view.copy_(codes)
  cu = torch.tensor(np.concatenate(([0], np.cumsum(qlens))), dtype=torch.int32, device="cuda")
  return dict(q=q, kv=kv, storage=storage, view=view, pool=view.view(F8), table=ids.cuda(), ids=ids, qlens=list(qlens), cache_list=list(cache), dtype=dtype, T=Tq,
              cache=torch.tensor(cache, dtype=torch.int32, device="cuda"), cu=cu, max_q=max(max(qlens), 1), capacity=pps * PAGE, page=PAGE)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("name", ["a", "b"])
@pytest.mark.parametrize("with_kv", [True, False])
def test_each_ragged_sequence_has_the_bits_of_the_uniform_call_on_it_alone(hip, dtype, name, with_kv):
  """The 16-bit tree suite's two ragged batches — token counts {1, 3, 0, 64, 7} (the full grid) and forty decodes + one 33-node tree (the compact grid, asserted
  from the plan) —, two rows of padding behind ``cu_seqlens_q[B]``, with the per-token quantising append and without it.  Sequence b with n_b tokens uses the
  top-left n_b x n_b of its mask: held to float64 on that sequence alone, and bit-identical to the uniform FP8 tree call on that sequence at the same forced
  number of KV ranges.  With ``kv=`` the storage afterwards is the torch-written one (``quantize_latent_rows`` at the append's places), byte for byte."""
  from ffpa_attn_amd import ffpa_attn_varlen_with_kvcache_mla_tree_fp8, ffpa_attn_with_kvcache_mla_tree_fp8

  qlens, kind, cache = RAGGED[name]
  hq, hkv, kv_scale = 16, 1, 0.37
  t = _ragged_case(qlens, cache, hq, hkv, dtype, seed=7)
  W = max(qlens)
  masks = _mask(kind, W, len(qlens), True, seed=W)
  words = masks.cuda()
  want_storage = t["storage"].clone()
  lens = _write_rows(t, want_storage, t["kv"][: t["T"]], cache, qlens, kv_scale) if with_kv else [min(c, t["capacity"]) for c in cache]
  want_pool = _pool_of(t, want_storage)
  for ns in (1, 3):
    storage = t["storage"].clone()
    pool = _pool_of(t, storage)
    with _launches(hip, hip.FLAG_FORCE_SPLITS if ns > 1 else 0) as plans:
      out, lse = ffpa_attn_varlen_with_kvcache_mla_tree_fp8(t["q"], pool, DV, t["cu"], t["max_q"], t["cache"], t["table"], kv_scale=kv_scale, tree_mask=words,
                                                            kv=t["kv"] if with_kv else None, softmax_scale=SCALE, num_splits=ns, return_softmax_lse=True)
    _the_new_kernel_and_no_other(plans, dtype)
    plan = plans[0]
    assert plan["splits"] == ns and out.shape == (t["q"].size(0), hq, DV) and lse.shape == (hq, t["q"].size(0))
    slots = hip.mla_compact_slots(hq // hkv, qlens)
    assert (slots > 0) == (name == "b") and plan["compact_slots"] == slots and ("compact grid" in plan["kernel"]) == (slots > 0), plan
    assert plan["workgroups"] == (slots if slots else len(qlens) * plan["row_tiles"]) * hkv * ns, plan
    assert _same_codes(storage, want_storage), "the cache's storage differs from the torch-written reference"
    if not with_kv:
      assert torch.equal(storage, t["storage"])
    row, seen, total = 0, 0, 0
    for b, n in enumerate(qlens):
      if n:
        tb, m = t["table"][b:b + 1], masks[b, :n, :n]
        qb = t["q"][row:row + n][None]
        deq = want_pool.double() * kv_scale
        o, l, pmax, p2sum = T.attend_tree(qb, deq, deq, [lens[b]], tb, m, SCALE)
        ref = (o[..., :DV].contiguous(), l, pmax, p2sum)
        assert not any(bool(torch.isnan(x).any()) for x in ref), "the reference holds NaN"
        seen += int(T.visible(m, 0, lens[b], n).any(dim=1).sum()) if lens[b] > 0 else 0
        total += n
        o_b, l_b = out[row:row + n][None], lse[:, row:row + n][None]
        R.check(o_b, l_b, ref, v=R.visible_values(deq[..., :DV], [lens[b]], tb), dtype=dtype,
                name=f"ragged {name} kv={with_kv} ranges {ns} sequence {b}: {n} tokens over {lens[b]} keys")
        empty = torch.isneginf(ref[1]).permute(0, 2, 1)
        assert (o_b[empty] == 0).all() and torch.isneginf(l_b.permute(0, 2, 1)[empty]).all()
        with _launches(hip, hip.FLAG_FORCE_SPLITS if ns > 1 else 0) as uplans:
          uo, ul = ffpa_attn_with_kvcache_mla_tree_fp8(qb, want_pool, DV, kv_scale=kv_scale, tree_mask=words[b:b + 1],
                                                       cache_seqlens=torch.tensor([lens[b]], dtype=torch.int32, device="cuda"), block_table=tb, softmax_scale=SCALE,
                                                       num_splits=ns, return_softmax_lse=True)
        _the_new_kernel_and_no_other(uplans, dtype)
        assert uplans[0]["splits"] == ns
        assert _same_bits(uo, o_b.contiguous()) and _same_bits(ul, l_b.contiguous()), f"sequence {b} ({n} tokens over {lens[b]} keys), {ns} ranges"
      row += n
    assert 4 * seen >= 3 * total, f"only {seen} of {total} query rows see a key"


# ----------------------------------------------------------------------------- 5. the append
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("snew", [1, 5])
@pytest.mark.parametrize("paged", [True, False])
@pytest.mark.parametrize("kv_scale", [0.37, 4.0])
def test_the_append_stores_quantize_latent_rows_at_its_places_and_nothing_else(hip, dtype, snew, paged, kv_scale):
  """``kv=`` at lengths 0, 31, 63 ... 65 (crossing a page) and 126 of 128 (rows at and past the capacity are dropped), paged and contiguous (capacity 128): the
  whole storage equals the one the torch helper wrote — the NaN pages around the pool included, NaN codes by NaN-ness —, exactly the appended rows changed, and
  the output is the call's on the pre-filled pool, bit for bit, and float64's.  The draft rows ARE the appended rows."""
  lens = [0, 31, 63, 64, 65, 126]
  t = _case(lens, 16, 1, snew, dtype, seed=40 + snew, pps=2, contiguous=0 if paged else 128)
  g = torch.Generator(device="cuda").manual_seed(177 + snew)
  kv = (torch.randn((len(lens), snew, 1, D), generator=g, device="cuda") * 3).to(R.TORCH_DTYPE[dtype])
  kv[0, 0, 0, :4] = torch.tensor([1e4, -1e4, float("inf"), 2.0 ** -10], dtype=kv.dtype)  # (saturating values and a tie to zero among the new rows)
  got, want = t["storage"].clone(), t["storage"].clone()
  used = _write_rows(t, want, kv.reshape(-1, 1, D), lens, [snew] * len(lens), kv_scale)
  assert used == [min(n + snew, 128) for n in lens]
  mask = _mask("tree" if snew > 1 else "ones", snew, len(lens), True, seed=snew)
  before = t["lens"].clone()
  out, lse, plan = _tree8(hip, t, mask, kv_scale=kv_scale, kv=kv, pool=_pool_of(t, got))
  assert torch.equal(t["lens"], before)  # (cache_seqlens is not advanced)
  assert _same_codes(got, want), "the cache's storage differs from the torch-written reference"
  touched = (want != t["storage"]).any(dim=-1).sum().item()
  assert touched == sum(u - n for u, n in zip(used, lens))  # (NaN rows became data: exactly the appended rows inside the capacity changed)
  again = _tree8(hip, t, mask, kv_scale=kv_scale, pool=_pool_of(t, want), lens=torch.tensor(used, dtype=torch.int32, device="cuda"))
  assert _same_out(out, again[0]) and _same_out(lse, again[1])
  ref, vstat = _ref(t, mask, kv_scale, lens=used, pool=_pool_of(t, want), guard=False)
  _hold(out, lse, ref, vstat, dtype, f"append Snew {snew} paged {paged} kv_scale {kv_scale}")


# ----------------------------------------------------------------------------- 6. one graph, torch.compile
def test_one_graph_over_a_split_launch_follows_words_lengths_table_and_new_rows(hip):
  """Quantising append + attention + merge (three forced ranges) captured once; replays after q, the mask words, cache_seqlens, block_table and kv were rewritten
  in place: each equals the eager call on the same state — storage included — and float64."""
  from ffpa_attn_amd import ffpa_attn_with_kvcache_mla_tree_fp8, pack_tree_mask

  lens0, sq = [5, 31, 64, 200], 5
  t = _case(lens0, 16, 1, sq, "bf16", seed=9, pps=5)
  storage = t["storage"].clone()
  storage[(storage & 0x7F) == 0x7F] = 0x30  # (replays move lengths and pages around: every row must hold a number)
  pool = _pool_of(t, storage)
  q, lens, table = t["q"].clone(), t["lens"].clone(), t["table"].clone()
  kv = torch.randn((4, sq, 1, D), device="cuda", dtype=torch.bfloat16)
  masks = [_mask(kind, sq, 4, True, seed=s) for s, kind in enumerate(("tree", "random", "sparse"))]
  words = pack_tree_mask(masks[0].cuda())
  call = lambda p: ffpa_attn_with_kvcache_mla_tree_fp8(q, p, DV, kv_scale=0.37, tree_mask=words, kv=kv, cache_seqlens=lens, block_table=table, softmax_scale=SCALE,
                                                       num_splits=3, return_softmax_lse=True)
  with _launches(hip, hip.FLAG_FORCE_SPLITS) as plans:
    call(pool.clone())  # (warm: the library is loaded, the scratch is sized)
  _the_new_kernel_and_no_other(plans, "bf16")
  assert plans[0]["splits"] == 3 and "ffpa_varlen_merge_kernel" in plans[0]["kernel"], plans[0]
  with _launches(hip, hip.FLAG_FORCE_SPLITS, record=False):
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
      out_g, lse_g = call(pool)
    states = [(lens0, table.clone(), kv.clone(), masks[0], q.clone()),
              ([0, 63, 65, 97], table.flip(0).contiguous(), torch.randn_like(kv), masks[1], torch.randn_like(q)),
              ([33, 1, 129, 300], table.roll(1, 0).contiguous(), torch.randn_like(kv), masks[2], torch.randn_like(q))]
    for n, tb, rows, mask, qq in states:
      lens.copy_(torch.tensor(n, dtype=torch.int32, device="cuda"))
      table.copy_(tb)
      kv.copy_(rows)
      q.copy_(qq)
      words.copy_(pack_tree_mask(mask.cuda()))
      snapshot = storage.clone()
      graph.replay()
      torch.cuda.synchronize()
      after = storage.clone()
      storage.copy_(snapshot)
      eager = call(pool)
      torch.cuda.synchronize()
      assert torch.equal(out_g, eager[0]) and torch.equal(lse_g, eager[1]), n
      assert torch.equal(after, storage) and not torch.equal(after, snapshot), n
      used = [x + sq for x in n]
      ref, vstat = _ref(t, mask, 0.37, lens=used, pool=pool, q=q, table=table, guard=False)
      _hold(out_g, lse_g, ref, vstat, "bf16", f"graph replay at {n}")


def test_the_uniform_call_under_torch_compile_fullgraph(hip):
  from ffpa_attn_amd import ffpa_attn_with_kvcache_mla_tree_fp8

  sq, lens = 3, [70, 2, 129]
  t = _case(lens, 16, 1, sq, "fp16", seed=88, pps=4)
  kv = torch.randn((3, sq, 1, D), device="cuda", dtype=torch.float16)
  mask = _mask("tree", sq, 3, True, seed=5)
  words = mask.cuda()

  def f(q, pool, rows, cache, table, words):
    o, lse = ffpa_attn_with_kvcache_mla_tree_fp8(q, pool, DV, kv_scale=0.37, tree_mask=words, kv=rows, cache_seqlens=cache, block_table=table, softmax_scale=SCALE,
                                                 return_softmax_lse=True)
    return o * 2, lse

  s_eager, s_compiled = t["storage"].clone(), t["storage"].clone()
  with _launches(hip) as plans:
    eager = f(t["q"], _pool_of(t, s_eager), kv, t["lens"], t["table"], words)
  _the_new_kernel_and_no_other(plans, "fp16")
  compiled = torch.compile(f, fullgraph=True)(t["q"], _pool_of(t, s_compiled), kv, t["lens"], t["table"], words)
  torch.cuda.synchronize()
  assert torch.equal(eager[0], compiled[0]) and torch.equal(eager[1], compiled[1])
  assert torch.equal(s_eager, s_compiled) and not torch.equal(s_eager, t["storage"])
  want = t["storage"].clone()
  used = _write_rows(t, want, kv.reshape(-1, 1, D), lens, [sq] * 3, 0.37)
  assert torch.equal(s_compiled, want)
  ref, vstat = _ref(t, mask, 0.37, lens=used, pool=_pool_of(t, want), guard=False)
  _hold((compiled[0].double() / 2).to(torch.float16), compiled[1], ref, vstat, "fp16", "torch.compile")
