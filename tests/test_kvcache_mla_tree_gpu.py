"""``ffpa_attn_with_kvcache_mla_tree`` / ``ffpa_attn_varlen_with_kvcache_mla_tree`` on the GPU: the latent kernel's tree build (``ffpa_fwd_m16_mla_tree_kernel``: the
MLA hook and the tree hook of the tile text both on) against the float64 restatement ``tree_ref.attend_tree(q, pool, pool, lens, table, mask, SCALE)[0][..., :512]``
through ``kvcache_ref.check`` (no tolerance of its own; LSE atol 2e-4 / rtol 2e-5), and bit for bit against the calls it must coincide with.  D = 576, head_dim_v =
512, scale 1 / sqrt(192), pages of 64 keys shuffled in a pool that holds NaN in every row no sequence owns.  Tiles: 64 rows x 32 keys, so the up to 64 draft keys
straddle up to three tiles and the draft window starts at any key modulo 32 — at key 0 (L == Sq) and below it (L < Sq) too.

Every case asserts ON THE REFERENCE that at least three quarters of its query rows see a key (counted as ``tree_ref.visible_rows`` counts them) and that the reference
holds no NaN; rows that see nothing are asserted exactly (O = 0, LSE = -inf)."""

import contextlib
import math
import random

import numpy as np
import pytest
import torch

import kvcache_ref as R
import tree_ref as T
from test_fwd_gpu import hip  # noqa: F401  (fixture)
from test_kvcache_mla_gpu import _case
from test_kvcache_mla_varlen_gpu import _case as _ragged_case, _write_rows

pytestmark = pytest.mark.gpu

D, DV, PAGE = 576, 512, 64
SCALE = 192 ** -0.5
HEADS = [(1, 1), (16, 1), (128, 1), (32, 2)]
TOKENS = [1, 2, 5, 33, 64]
KERNEL = "ffpa_fwd_m16_mla_tree_kernel"


def _lens(sq):
  """0, L < Sq, L == Sq (the draft window starts at key 0), Sq + 1, both sides of one and two 32-key tiles, an odd tile count, ten tiles.  At Sq = 64 the lengths
  31 ... 33 lie below Sq as well and a TREE mask (a node sees ancestors only) leaves 161 of these nine sequences' 576 rows without a key whatever the tree: two
  longer sequences more bring the batch to the three quarters every case must show."""
  return sorted({0, sq - 1, sq, sq + 1, 31, 32, 33, 64, 65, 97, 300} | ({129, 200} if sq == 64 else set()))


def _mask(kind, sq, B, per_sequence, seed):
  """A mask of ``tree_ref.MASK_KINDS`` on the CPU: ``[Sq, Sq]``, or ``[B, Sq, Sq]`` with ``per_sequence``."""
  rng = random.Random(seed * 977 + 5)
  if per_sequence:
    return torch.stack([T.draw_mask(kind, sq, rng) for _ in range(B)])
  return T.draw_mask(kind, sq, rng)


@contextlib.contextmanager
def _launches(hip, flags=0):
  """Every tree latent launch inside the block carries ``flags`` too and its plan is appended to the list the block receives; a latent launch WITHOUT mask words
  inside the block is recorded as a stray."""
  plans, strays, real, inner = [], [], hip.mla_tree_forward, hip.mla_forward

  def spy(*args, **kw):
    plan = {}
    kw["flags"] = kw.get("flags", 0) | flags
    kw["plan_out"] = plan
    out = real(*args, **kw)
    plans.append(plan)
    return out

  def watch(*args, **kw):
    if kw.get("tree_words") is None:
      strays.append("mla_forward without tree_words")
    return inner(*args, **kw)

  hip.mla_tree_forward, hip.mla_forward = spy, watch
  try:
    yield plans
  finally:
    hip.mla_tree_forward, hip.mla_forward = real, inner
  assert not strays, strays


def _the_new_kernel_and_no_other(plans, dtype, n=1):
  assert len(plans) == n and all(p["kernel"].startswith(f"{KERNEL}<{dtype}, 576, dv=512") for p in plans), plans


def _tree(hip, t, mask, *, num_splits=0, flags=0, lens=None, kv=None, pool=None, q=None, table="case"):
  from ffpa_attn_amd import ffpa_attn_with_kvcache_mla_tree

  with _launches(hip, flags) as plans:
    out, lse = ffpa_attn_with_kvcache_mla_tree(t["q"] if q is None else q, t["pool"] if pool is None else pool, DV, tree_mask=mask.cuda(), kv=kv,
                                               cache_seqlens=t["lens"] if lens is None else lens, block_table=t["table"] if isinstance(table, str) else table,
                                               softmax_scale=SCALE, num_splits=num_splits, return_softmax_lse=True)
  _the_new_kernel_and_no_other(plans, t["dtype"])
  return out, lse, plans[0]


def _ref(t, mask, lens=None, pool=None, q=None, table="case"):
  """The issue's reference: float64 tree attention on (pool, pool), value columns ``[:512]``; with the two conditions on the inputs asserted on it."""
  pool = t["pool"] if pool is None else pool
  q = t["q"] if q is None else q
  lens = t["lens_list"] if lens is None else lens
  table = t["table"] if isinstance(table, str) else table
  o, lse, pmax, p2sum = T.attend_tree(q, pool, pool, lens, table, mask, SCALE)
  ref = (o[..., :DV].contiguous(), lse, pmax, p2sum)
  sq, cap = q.size(1), R.capacity_of(pool, table)
  seen = sum(int(T.visible(mask, b, min(max(int(n), 0), cap), sq).any(dim=1).sum()) for b, n in enumerate(lens) if min(max(int(n), 0), cap) > 0)
  assert 4 * seen >= 3 * len(lens) * sq, f"only {seen} of {len(lens) * sq} query rows see a key: the case could hide a failure behind empty rows"
  assert not any(bool(torch.isnan(x).any()) for x in ref), "the reference holds NaN"
  empty = torch.isneginf(lse)  # [B, Hq, Sq]
  assert int(empty[:, 0].sum()) == len(lens) * sq - seen
  return ref


def _hold(out, lse, ref, vstat, dtype, name):
  ratio = R.check(out, lse, ref, v=vstat, dtype=dtype, name=name)
  empty = torch.isneginf(ref[1]).permute(0, 2, 1)  # [B, Sq, Hq]: rows that see nothing, exactly
  assert (out[empty] == 0).all() and torch.isneginf(lse.permute(0, 2, 1)[empty]).all(), name
  print(f"[mla tree] {ratio:.3f} {name}")
  return ratio


def _check(hip, t, mask, what, **kw):
  ref = _ref(t, mask)
  out, lse, plan = _tree(hip, t, mask, **kw)
  name = f"{what}: {t['dtype']} heads {t['heads']} Sq {t['sq']} lens {t['lens_list']} {kw} -> {plan}"
  assert out.shape == (len(t["lens_list"]), t["sq"], t["heads"][0], DV) and lse.shape == (len(t["lens_list"]), t["heads"][0], t["sq"])
  _hold(out, lse, ref, t["vstat"], t["dtype"], name)
  return out, lse, plan, ref


def _same(got, want, dtype, what=""):
  """LSE bit for bit in both dtypes; O bit for bit in bf16, within one output ulp in fp16."""
  assert torch.equal(got[1], want[1]), f"{what}: LSE differs"
  if dtype == "bf16":
    assert torch.equal(got[0], want[0]), f"{what}: {int((got[0] != want[0]).sum())} elements differ, max {(got[0].float() - want[0].float()).abs().max().item():.3e}"
  else:
    assert ((got[0].double() - want[0].double()).abs() <= R.ulp_of(want[0].double(), dtype)).all(), what


# ----------------------------------------------------------------------------- key lengths x heads x tokens x masks
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("hq, hkv, sq", [(hq, hkv, sq) for hq, hkv in HEADS for sq in TOKENS] + [(128, 1, 3)])
@pytest.mark.parametrize("kind", ["tree", "random", "sparse"])
def test_key_lengths_heads_tokens_and_masks(hip, dtype, hq, hkv, sq, kind):
  """The lengths of ``_lens`` as ONE batch.  The group's heads x tokens are the rows of ceil(group x Sq / 64) chunks: (16, 1) x 5 puts a chunk boundary inside a head,
  (128, 1) x 3 spans six chunks; (1, 1) runs unpacked.  ``random`` clears diagonals, sees later nodes and has an all-False row; ``sparse`` sets bit Sq - 1 (bit 63
  at Sq 64).  Per-sequence and shared masks alternate over the cases."""
  lens = _lens(sq)
  t = _case(lens, hq, hkv, sq, dtype, seed=hq + sq)
  per_sequence = (hq + sq + len(kind)) % 2 == 0
  mask = _mask(kind, sq, len(lens), per_sequence, seed=sq + hq)
  out, lse, plan, ref = _check(hip, t, mask, f"{kind} {'per sequence' if per_sequence else 'shared'}")
  group = hq // hkv
  assert plan["block_rows"] == 64 and plan["block_keys"] == 32
  assert plan["row_tiles"] == (math.ceil(group * sq / 64) if group > 1 else 1), plan
  assert plan["workgroups"] == len(lens) * hkv * plan["row_tiles"] * plan["splits"], plan
  assert ("packed into rows" in plan["kernel"]) == (group > 1) and ("chunked" in plan["kernel"]) == (group * sq > 64 and group > 1), plan
  assert (out[0] == 0).all() and torch.isneginf(lse[0]).all()  # (L = 0)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("hq, hkv", [(16, 1), (128, 1), (1, 1)])
def test_one_token_keeps_its_mask(hip, dtype, hq, hkv):
  """``[[False]]`` hides the token's own row — the launch keeps the causal flag at one token per sequence: such a token sees the prefix only, nothing at L = 1."""
  lens = _lens(1)
  t = _case(lens, hq, hkv, 1, dtype, seed=hq + 1)
  mask = torch.tensor([[[b % 2 == 0]] for b in range(len(lens))])  # (L = 1 has [[False]]: an empty row)
  assert lens[1] == 1 and not bool(mask[1, 0, 0])
  out, lse, plan, ref = _check(hip, t, mask, "one token")
  assert (out[1] == 0).all() and torch.isneginf(lse[1]).all()
  shared = torch.zeros(1, 1, dtype=torch.bool)
  t2 = _case([2, 33, 64, 65, 300], hq, hkv, 1, dtype, seed=hq + 2)
  _check(hip, t2, shared, "one token, [[False]] for all")


# ----------------------------------------------------------------------------- the calls it must coincide with
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("hq, hkv, sq", [(16, 1, 1), (16, 1, 3), (16, 1, 5), (128, 1, 3), (32, 2, 33), (1, 1, 5), (16, 1, 64)])
def test_tril_is_the_causal_latent_call_and_all_ones_the_plain_one(hip, dtype, hq, hkv, sq):
  from ffpa_attn_amd import ffpa_attn_with_kvcache_mla

  lens = _lens(sq)
  t = _case(lens, hq, hkv, sq, dtype, seed=hq + sq)
  for causal, mask in ((True, torch.ones(sq, sq, dtype=torch.bool).tril()), (False, torch.ones(sq, sq, dtype=torch.bool))):
    got = _tree(hip, t, mask, num_splits=1)
    want = ffpa_attn_with_kvcache_mla(t["q"], t["pool"], DV, cache_seqlens=t["lens"], block_table=t["table"], softmax_scale=SCALE, causal=causal, num_splits=1,
                                      return_softmax_lse=True)
    _same(got, want, dtype, f"causal={causal}")
    # ... per sequence, as packed words, and as a mask wider than the batch's tokens (W = 64: the top-left Sq x Sq is read)
    from ffpa_attn_amd import pack_tree_mask

    wide = torch.zeros(64, 64, dtype=torch.bool)
    wide[:sq, :sq] = mask
    wide[:sq, sq:] = True  # (bits past the sequence's tokens are never tested)
    for form in (mask[None].expand(len(lens), sq, sq).contiguous(), pack_tree_mask(mask.cuda()), wide, pack_tree_mask(wide.cuda())):
      again = _tree(hip, t, form, num_splits=1)
      assert torch.equal(again[0], got[0]) and torch.equal(again[1], got[1])


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("sq", [1, 3])
@pytest.mark.parametrize("kind", ["tree", "random"])
def test_same_arithmetic_as_the_two_cache_tree_call_on_the_aliased_pool(hip, dtype, sq, kind):
  """``ffpa_attn_with_kvcache_tree(q, kv, kv)[..., :512]`` packs the 16 heads x Sq tokens into the rows of one tile as this call does."""
  from ffpa_attn_amd import ffpa_attn_with_kvcache_tree

  lens = _lens(sq)
  t = _case(lens, 16, 1, sq, dtype, seed=16 + sq)
  mask = _mask(kind, sq, len(lens), True, seed=sq) if sq > 1 else torch.tensor([[[b % 3 != 0]] for b in range(len(lens))])
  got = _tree(hip, t, mask, num_splits=1)
  want, want_lse = ffpa_attn_with_kvcache_tree(t["q"], t["pool"], t["pool"], cache_seqlens=t["lens"], block_table=t["table"], tree_mask=mask.cuda(),
                                               softmax_scale=SCALE, num_splits=1, return_softmax_lse=True)
  _same(got, (want[..., :DV], want_lse), dtype, "two-cache tree call")


# ----------------------------------------------------------------------------- KV ranges
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("hq, hkv, sq", [(16, 1, 2), (128, 1, 5)])
def test_forced_kv_ranges_start_at_odd_tiles(hip, dtype, hq, hkv, sq):
  """num_splits 1, 2, 3 and 5 forced on the batch: every sequence shares out ITS tiles (1 ... 10 of 32 keys), so ranges start at odd tiles and both image parities
  meet the branch; with five ranges over two or three tiles some ranges are empty.  Every count agrees with float64 and with the unsplit launch to the merge's
  rounding (two allowances); the library's own count is one of them, bit for bit."""
  lens = _lens(sq)
  t = _case(lens, hq, hkv, sq, dtype, seed=hq + sq)
  mask = _mask("random", sq, len(lens), True, seed=3 * sq)
  outs = {}
  for ns in (1, 2, 3, 5):
    out, lse, plan, ref = _check(hip, t, mask, "KV ranges", num_splits=ns, flags=hip.FLAG_FORCE_SPLITS)
    assert plan["splits"] == ns, plan
    assert ("ffpa_varlen_merge_kernel" in plan["kernel"]) == (ns > 1)
    outs[ns] = (out, lse)
  o_ref, lse_ref, pmax, p2sum = (x.cpu().numpy() for x in ref)
  stat = lambda x: np.transpose(x, (0, 2, 1))
  half_ulp, flip = R.allowance(o_ref, stat(pmax), stat(p2sum), t["vstat"], dtype, noise=True)
  for ns in (2, 3, 5):
    err = (outs[ns][0].double() - outs[1][0].double()).abs().cpu().numpy()
    assert (err <= 2 * (half_ulp + flip)).all(), f"num_splits {ns} vs 1: {err.max():.3e}"
    torch.testing.assert_close(outs[ns][1], outs[1][1], atol=2 * R.LSE_ATOL, rtol=2 * R.LSE_RTOL)
  out0, lse0, plan0, _ = _check(hip, t, mask, "library's own count")
  same = [ns for ns in outs if torch.equal(out0, outs[ns][0]) and torch.equal(lse0, outs[ns][1])]
  forced = None
  if not same:  # (the heuristic's own count, forced)
    forced = _tree(hip, t, mask, num_splits=plan0["splits"], flags=hip.FLAG_FORCE_SPLITS)
    same = [plan0["splits"]] if torch.equal(out0, forced[0]) and torch.equal(lse0, forced[1]) else []
  assert same, (plan0, forced[2] if forced else None)


# ----------------------------------------------------------------------------- the NT build
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("hq, hkv, sq", [(16, 1, 2), (16, 1, 5), (1, 1, 5)])
def test_the_nt_build_is_bit_identical_to_the_plain_build(hip, dtype, hq, hkv, sq):
  lens = _lens(sq)
  t = _case(lens, hq, hkv, sq, dtype, seed=hq + sq)
  mask = _mask("tree", sq, len(lens), False, seed=sq)
  for ns in (1, 3):
    force = hip.FLAG_FORCE_SPLITS if ns > 1 else 0
    plain = _tree(hip, t, mask, num_splits=ns, flags=force | hip.FLAG_NO_KV_STREAM)
    nt = _tree(hip, t, mask, num_splits=ns, flags=force | hip.FLAG_KV_STREAM)
    assert ", NT>" in nt[2]["kernel"] and ", NT>" not in plain[2]["kernel"], (plain[2], nt[2])
    assert torch.equal(plain[0], nt[0]) and torch.equal(plain[1], nt[1])
  _hold(nt[0], nt[1], _ref(t, mask), t["vstat"], dtype, f"NT build {dtype} heads {(hq, hkv)} Sq {sq}")


# ----------------------------------------------------------------------------- the append
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("snew", [1, 5])
@pytest.mark.parametrize("paged", [True, False])
def test_append_writes_each_latent_row_once_and_nothing_else(hip, dtype, snew, paged):
  """``kv=`` at lengths 0, 31 and 63 ... 65 (crossing a page) equals writing the rows with torch and then attending; the storage — NaNs included — is the same
  integers as the reference's everywhere.  The draft rows ARE the appended rows."""
  lens = [0, 31, 63, 64, 65]
  t = _case(lens, 16, 1, snew, dtype, seed=40 + snew, room=8, contiguous=0 if paged else 128)
  g = torch.Generator(device="cuda").manual_seed(77 + snew)
  kv = torch.randn((len(lens), snew, 1, D), generator=g, device="cuda", dtype=R.TORCH_DTYPE[dtype])
  got_storage, want_storage = t["storage"].clone(), t["storage"].clone()
  got_pool, want_pool = R.reviewed(t["pool"], t["storage"], got_storage), R.reviewed(t["pool"], t["storage"], want_storage)
  _, used, _ = R.append(want_pool, want_pool, kv, kv, lens, t["table"])
  assert used == [n + snew for n in lens]
  mask = _mask("tree" if snew > 1 else "ones", snew, len(lens), True, seed=snew)
  before = t["lens"].clone()
  out, lse, plan = _tree(hip, t, mask, kv=kv, pool=got_pool)
  assert torch.equal(t["lens"], before)  # (cache_seqlens is not advanced)
  assert torch.equal(got_storage.view(torch.int16), want_storage.view(torch.int16)), "the cache's storage differs from the torch-written reference"
  touched = (want_storage.view(torch.int16) != t["storage"].view(torch.int16)).any(dim=-1).sum().item()
  assert touched == len(lens) * snew  # (NaN rows became data: exactly the appended rows changed)
  ref = _ref(t, mask, lens=used, pool=want_pool)
  _hold(out, lse, ref, R.visible_values(want_pool[..., :DV], used, t["table"]), dtype, f"append Snew {snew} paged {paged}")
  # ... and attending over the written cache without kv= gives the same bits
  again = _tree(hip, t, mask, pool=got_pool, lens=torch.tensor(used, dtype=torch.int32, device="cuda"))
  assert torch.equal(out, again[0]) and torch.equal(lse, again[1])


# ----------------------------------------------------------------------------- the contiguous cache
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_a_contiguous_cache_of_capacity_128(hip, dtype):
  from ffpa_attn_amd import ffpa_attn_with_kvcache_mla_tree

  t = _case([5, 97, 128], 16, 1, 5, dtype, seed=6, contiguous=128)
  assert t["table"] is None and t["pool"].shape == (3, 128, 1, D)
  mask = _mask("random", 5, 3, True, seed=11)
  _check(hip, t, mask, "contiguous")
  with pytest.raises(ValueError, match="multiple of 64"):
    ffpa_attn_with_kvcache_mla_tree(t["q"], t["pool"][:, :100], DV, tree_mask=mask.cuda(), cache_seqlens=t["lens"], softmax_scale=SCALE)


# ----------------------------------------------------------------------------- ragged batches
# (token counts, mask kind, cache lengths before the step: a one-token sequence on an empty cache — with the append its draft window starts at key 0 —, both sides
# of a tile, an odd tile count, ten tiles)
RAGGED = {"a": ([1, 3, 0, 64, 7], "tree", [0, 33, 300, 97, 31]), "b": ([1] * 40 + [33], "random", [(0, 1, 31, 33, 64, 97, 300)[b % 7] for b in range(40)] + [97])}


def _ragged_reference(t, masks, with_kv):
  want_storage = t["storage"].clone()
  want_pool = R.reviewed(t["pool"], t["storage"], want_storage)
  lens = _write_rows(t, want_pool) if with_kv else [min(max(c, 0), t["capacity"]) for c in t["cache_list"]]
  per_seq, row, seen, total = {}, 0, 0, 0
  for b, n in enumerate(t["qlens"]):
    if n:
      tb = None if t["table"] is None else t["table"][b:b + 1]
      m = masks[b, :n, :n]
      o, lse, pmax, p2sum = T.attend_tree(t["q"][row:row + n][None], want_pool, want_pool, [lens[b]], tb, m, SCALE)
      ref = (o[..., :DV].contiguous(), lse, pmax, p2sum)
      assert not any(bool(torch.isnan(x).any()) for x in ref), "the reference holds NaN"
      per_seq[b] = (ref, R.visible_values(want_pool[..., :DV], [lens[b]], tb))
      seen += int(T.visible(m, 0, lens[b], n).any(dim=1).sum()) if lens[b] > 0 else 0
      total += n
    row += n
  assert 4 * seen >= 3 * total, f"only {seen} of {total} query rows see a key"
  return per_seq, want_pool, want_storage, lens


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("name", ["a", "b"])
@pytest.mark.parametrize("with_kv", [True, False])
def test_ragged_batches_per_sequence_against_float64_and_the_uniform_call(hip, dtype, name, with_kv):
  """Token counts {1, 3, 0, 64, 7} (the full grid) and forty decodes + one 33-node tree (the compact grid, asserted from the plan), two rows of padding behind
  ``cu_seqlens_q[B]``, with the per-token append and without it.  Sequence b with n_b tokens uses the top-left n_b x n_b of its mask: held to float64 on that
  sequence alone, and bit-identical to the uniform tree call on that sequence at the same forced number of KV ranges."""
  from ffpa_attn_amd import ffpa_attn_varlen_with_kvcache_mla_tree, ffpa_attn_with_kvcache_mla_tree

  qlens, kind, cache = RAGGED[name]
  hq, hkv = 16, 1
  t = _ragged_case(qlens, hq, hkv, dtype, seed=7, cache=cache, pad=2, room=8)
  W = max(qlens)
  masks = _mask(kind, W, len(qlens), True, seed=W)
  per_seq, want_pool, want_storage, lens = _ragged_reference(t, masks, with_kv)
  words = masks.cuda()
  for ns in (1, 3):
    storage = t["storage"].clone()
    pool = R.reviewed(t["pool"], t["storage"], storage)
    with _launches(hip, hip.FLAG_FORCE_SPLITS if ns > 1 else 0) as plans:
      out, lse = ffpa_attn_varlen_with_kvcache_mla_tree(t["q"], pool, DV, t["cu"], t["max_q"], t["cache"], t["table"], tree_mask=words, kv=t["kv"] if with_kv else None,
                                                        softmax_scale=SCALE, num_splits=ns, return_softmax_lse=True)
    _the_new_kernel_and_no_other(plans, dtype)
    plan = plans[0]
    assert plan["splits"] == ns and out.shape == (t["q"].size(0), hq, DV) and lse.shape == (hq, t["q"].size(0))
    slots = hip.mla_compact_slots(hq // hkv, qlens)
    assert (slots > 0) == (name == "b") and plan["compact_slots"] == slots and ("compact grid" in plan["kernel"]) == (slots > 0), plan
    assert plan["workgroups"] == (slots if slots else len(qlens) * plan["row_tiles"]) * hkv * ns, plan
    if with_kv:  # (the per-token append: the storage is the torch-written reference's, NaNs and the padding rows' absence included)
      assert torch.equal(storage.view(torch.int16), want_storage.view(torch.int16))
    else:
      assert torch.equal(storage.view(torch.int16), t["storage"].view(torch.int16))
    row = 0
    for b, n in enumerate(qlens):
      if n:
        ref, vstat = per_seq[b]
        o_b, l_b = out[row:row + n][None], lse[:, row:row + n][None]
        R.check(o_b, l_b, ref, v=vstat, dtype=dtype, name=f"ragged {name} kv={with_kv} ranges {ns} sequence {b}: {n} tokens over {lens[b]} keys")
        empty = torch.isneginf(ref[1]).permute(0, 2, 1)
        assert (o_b[empty] == 0).all() and torch.isneginf(l_b.permute(0, 2, 1)[empty]).all()
        with _launches(hip, hip.FLAG_FORCE_SPLITS if ns > 1 else 0) as uplans:
          uo, ul = ffpa_attn_with_kvcache_mla_tree(t["q"][row:row + n][None], want_pool if with_kv else t["pool"], DV, tree_mask=words[b:b + 1],
                                                   cache_seqlens=torch.tensor([lens[b]], dtype=torch.int32, device="cuda"),
                                                   block_table=None if t["table"] is None else t["table"][b:b + 1], softmax_scale=SCALE, num_splits=ns,
                                                   return_softmax_lse=True)
        _the_new_kernel_and_no_other(uplans, dtype)
        assert uplans[0]["splits"] == ns
        assert torch.equal(uo, o_b) and torch.equal(ul, l_b), f"sequence {b} ({n} tokens over {lens[b]} keys), {ns} ranges"
      row += n


# ----------------------------------------------------------------------------- host paths
def test_one_graph_over_a_split_launch_follows_words_lengths_table_and_new_rows(hip):
  """Append + attention + merge (three forced ranges) captured once; replays after the mask words, cache_seqlens, block_table and kv were rewritten in place: each
  equals the eager call on the same state and float64."""
  from ffpa_attn_amd import ffpa_attn_with_kvcache_mla_tree, pack_tree_mask

  lens0, sq = [5, 31, 64, 200], 5
  t = _case(lens0, 16, 1, sq, "bf16", seed=9, room=16)
  storage = t["storage"].clone()
  pool = R.reviewed(t["pool"], t["storage"], storage)
  pool.nan_to_num_(nan=0.25)  # (replays move lengths and pages around: every row must hold a number)
  lens, table = t["lens"].clone(), t["table"].clone()
  kv = torch.randn((4, sq, 1, D), device="cuda", dtype=torch.bfloat16)
  masks = [_mask(kind, sq, 4, True, seed=s) for s, kind in enumerate(("tree", "random", "sparse"))]
  words = pack_tree_mask(masks[0].cuda())
  call = lambda p: ffpa_attn_with_kvcache_mla_tree(t["q"], p, DV, tree_mask=words, kv=kv, cache_seqlens=lens, block_table=table, softmax_scale=SCALE, num_splits=3,
                                                   return_softmax_lse=True)
  with _launches(hip, hip.FLAG_FORCE_SPLITS) as plans:
    call(pool.clone())  # (warm: the library is loaded, the scratch is sized)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
      out_g, lse_g = call(pool)
    _the_new_kernel_and_no_other(plans, "bf16", 2)
    assert plans[1]["splits"] == 3 and "ffpa_varlen_merge_kernel" in plans[1]["kernel"], plans[1]
    states = [(lens0, table.clone(), kv.clone(), masks[0]),
              ([0, 63, 65, 97], table.flip(0).contiguous(), torch.randn_like(kv), masks[1]),
              ([33, 1, 129, 300], table.roll(1, 0).contiguous(), torch.randn_like(kv), masks[2])]
    for n, tb, rows, mask in states:
      lens.copy_(torch.tensor(n, dtype=torch.int32, device="cuda"))
      table.copy_(tb)
      kv.copy_(rows)
      words.copy_(pack_tree_mask(mask.cuda()))
      snapshot = storage.clone()
      graph.replay()
      torch.cuda.synchronize()
      after = storage.clone()
      storage.copy_(snapshot)
      eager = call(pool)
      torch.cuda.synchronize()
      assert torch.equal(out_g, eager[0]) and torch.equal(lse_g, eager[1]), n
      assert torch.equal(after.view(torch.int16), storage.view(torch.int16)), n
      used = [x + sq for x in n]
      ref = _ref(t, mask, lens=used, pool=pool, table=table)
      _hold(out_g, lse_g, ref, R.visible_values(pool[..., :DV], used, table), "bf16", f"graph replay at {n}")


def test_under_torch_compile_fullgraph(hip):
  from ffpa_attn_amd import ffpa_attn_with_kvcache_mla_tree

  sq, lens = 3, [70, 2, 129]
  t = _case(lens, 16, 1, sq, "fp16", seed=88, room=8)
  kv = torch.randn((3, sq, 1, D), device="cuda", dtype=torch.float16)
  mask = _mask("tree", sq, 3, True, seed=5)
  words = mask.cuda()

  def f(q, pool, kv, lens, table, words):
    o, lse = ffpa_attn_with_kvcache_mla_tree(q, pool, DV, tree_mask=words, kv=kv, cache_seqlens=lens, block_table=table, softmax_scale=SCALE, return_softmax_lse=True)
    return o * 2, lse

  s_eager, s_compiled = t["storage"].clone(), t["storage"].clone()
  p_eager, p_compiled = R.reviewed(t["pool"], t["storage"], s_eager), R.reviewed(t["pool"], t["storage"], s_compiled)
  with _launches(hip) as plans:
    eager = f(t["q"], p_eager, kv, t["lens"], t["table"], words)
  _the_new_kernel_and_no_other(plans, "fp16")
  compiled = torch.compile(f, fullgraph=True)(t["q"], p_compiled, kv, t["lens"], t["table"], words)
  torch.cuda.synchronize()
  assert torch.equal(eager[0], compiled[0]) and torch.equal(eager[1], compiled[1])
  assert torch.equal(s_eager.view(torch.int16), s_compiled.view(torch.int16)) and not torch.equal(s_eager.view(torch.int16), t["storage"].view(torch.int16))
  used = [n + sq for n in lens]
  want = t["storage"].clone()
  wp = R.reviewed(t["pool"], t["storage"], want)
  R.append(wp, wp, kv, kv, lens, t["table"])
  assert torch.equal(s_compiled.view(torch.int16), want.view(torch.int16))
  _hold((compiled[0].double() / 2).to(torch.float16), compiled[1], _ref(t, mask, lens=used, pool=wp), R.visible_values(wp[..., :DV], used, t["table"]), "fp16",
        "torch.compile")


@pytest.mark.parametrize("num_splits", [1, 3])
def test_a_side_stream_gives_the_bits_of_the_current_stream(hip, num_splits):
  sq, lens = 2, [5, 200, 1000, 64]
  t = _case(lens, 16, 1, sq, "bf16", seed=89, room=8)
  kv = torch.randn((4, sq, 1, D), device="cuda", dtype=torch.bfloat16)
  mask = _mask("random", sq, 4, True, seed=2)
  s_main, s_side = t["storage"].clone(), t["storage"].clone()
  kw = dict(kv=kv, num_splits=num_splits, flags=hip.FLAG_FORCE_SPLITS if num_splits > 1 else 0)
  main = _tree(hip, t, mask, pool=R.reviewed(t["pool"], t["storage"], s_main), **kw)
  torch.cuda.synchronize()
  stream = torch.cuda.Stream()
  assert stream != torch.cuda.current_stream()
  with torch.cuda.stream(stream):
    side = _tree(hip, t, mask, pool=R.reviewed(t["pool"], t["storage"], s_side), **kw)
  stream.synchronize()
  assert side[2] == main[2] and main[2]["splits"] == num_splits, (main[2], side[2])
  assert torch.equal(main[0], side[0]) and torch.equal(main[1], side[1])
  assert torch.equal(s_main.view(torch.int16), s_side.view(torch.int16)) and not torch.equal(s_main.view(torch.int16), t["storage"].view(torch.int16))
  used = [n + sq for n in lens]
  wp = R.reviewed(t["pool"], t["storage"], s_main)
  _hold(main[0], main[1], _ref(t, mask, lens=used, pool=wp), R.visible_values(wp[..., :DV], used, t["table"]), "bf16", f"side stream, {num_splits} ranges")
