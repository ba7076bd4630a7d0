"""Shared-prefix (cascade) attention over the MLA latent cache on the GPU: the plan kernel against its torch restatement (tests/kvcache_mla_cascade_ref.py),
exactly; ffpa_attn_with_kvcache_mla_cascade against float64 attention over the gathered keys (tests/kvcache_ref.py ``attend``) and against the plain latent call,
by the rule of tests/test_cascade_gpu.py — no element further from float64 than the plain call's largest error on the case plus one ulp of the output dtype at the
reference, no NaN, LSE finite in the same places and within 1e-3; a zero prefix and cascade=False bit-identical to the plain call; the prefix read through every
group's first sequence only; a stated prefix longer than a sequence; the kv= append; the FP8 twin; one HIP graph with everything written in place; torch.compile
and opcheck.  Shapes: pages of 64 and 128 rows, 128 ... 256 shared keys (4 ... 8 tiles of 32 keys), 5 ... 6 sequences, 16 and 128 query heads over one latent head
(one and several row chunks per group), 1 and 3 query tokens."""

import math

import pytest
import torch

import kvcache_ref as R
from kvcache_mla_cascade_ref import plan as ref_plan
from test_fwd_gpu import hip  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

D, DV = 576, 512
SCALE = 192 ** -0.5


def _groups_of(sizes):
  cu = [0]
  for n in sizes:
    cu.append(cu[-1] + n)
  return cu


def _case(sizes, share, lens, hq, dtype, page, seed, sq=1, diverge=False, nan_unused=True, extra_pages=0):
  """B = sum(sizes) sequences in groups of ``sizes`` consecutive ones; the sequences of group g share their first ``share[g]`` keys (a page multiple): the same
  page ids in the first ``share[g] / page`` columns of their block-table rows — with ``diverge``, every sequence but the group's first points at OTHER pages of
  other content there.  Sequence b holds ``lens[b]`` keys.  Pages no sequence reads, and rows past a length, hold NaN.  -> dict: q, pool, table, truth (the
  table with every shared column taken from the group's first sequence: what the answer is defined by), lens, cu (the groups' boundaries), cap."""
  g = torch.Generator(device="cuda").manual_seed(seed)
  cu = _groups_of(sizes)
  B = cu[-1]
  W = max(-(-max(lens) // page), max(share) // page) + 1 + extra_pages
  n_pages = 0
  rows, truth_rows = [], []
  for gi, n in enumerate(sizes):
    npre = share[gi] // page
    shared = list(range(n_pages, n_pages + npre))
    n_pages += npre
    for i in range(n):
      if diverge and i > 0:
        pre = list(range(n_pages, n_pages + npre))
        n_pages += npre
      else:
        pre = shared
      own = list(range(n_pages, n_pages + W - npre))
      n_pages += W - npre
      rows.append(pre + own)
      truth_rows.append(shared + own)
  n_pages += 3
  perm = torch.randperm(n_pages, generator=torch.Generator().manual_seed(seed))
  table = perm[torch.tensor(rows)].to(torch.int32)
  truth = perm[torch.tensor(truth_rows)].to(torch.int32)
  pool = (torch.randn((n_pages, page, 1, D), generator=g, device="cuda") * 0.5).to(dtype)
  if nan_unused:
    used = torch.zeros((n_pages, page), dtype=torch.bool)
    for b in range(B):
      n = min(max(lens[b], 0), W * page)
      j = torch.arange(n)
      used[truth[b].long()[j // page], j % page] = True
      if diverge:  # (the other content stays data: reading it would give a finite, wrong answer; only what nobody may read is NaN)
        used[table[b].long()[j // page], j % page] = True
    pool[(~used).cuda()] = float("nan")
  q = torch.randn((B, sq, hq, D), generator=g, device="cuda").to(dtype)
  return dict(q=q, pool=pool, table=table.cuda(), truth=truth.cuda(), lens=torch.tensor(lens, dtype=torch.int32, device="cuda"), cu=cu, cap=W * page, page=page,
              cu_t=torch.tensor(cu, dtype=torch.int32, device="cuda"))


def _float64(t, causal, lens=None, pool=None, q=None):
  pool = (t["pool"] if pool is None else pool).double()
  o, lse, _, _ = R.attend(t["q"] if q is None else q, pool, pool, t["lens"].tolist() if lens is None else lens, t["truth"], causal, SCALE)
  return o[..., :DV], lse


def _check_accuracy(cas, lse_c, plain, ref, ref_lse, dtype):
  """tests/test_cascade_gpu.py ``_check_accuracy``, with the LSE."""
  err_p = (plain.double() - ref).abs().max()
  err_c = (cas.double() - ref).abs()
  bound = err_p + R.ulp_of(ref, dtype)
  assert not torch.isnan(cas).any()
  assert (err_c <= bound).all(), f"cascade max err {err_c.max().item():.3e}, plain max err {err_p.item():.3e}"
  if lse_c is not None:
    fin = torch.isfinite(ref_lse)
    assert torch.equal(torch.isfinite(lse_c), fin) and (lse_c[~fin] == -math.inf).all()
    assert ((lse_c.double() - ref_lse)[fin].abs() <= 1e-3).all(), (lse_c.double() - ref_lse)[fin].abs().max()


def _suffixes(sq, n):
  return [0, 1, sq, 70, 129, 200][:n]


# ---- the plan kernel
def _plan_both(lens, table, cu_g, spl, page, sq, causal, cap):
  dev_spl = spl if isinstance(spl, torch.Tensor) else None
  got = torch.ops.ffpa_attn._mla_cascade_plan_hip(lens, table, cu_g, dev_spl, 0 if dev_spl is not None else spl, page, sq, 1 if causal else 0, cap)
  torch.cuda.synchronize()
  want = ref_plan(lens.cpu(), table.cpu(), None if cu_g is None else cu_g.cpu(), spl.cpu() if dev_spl is not None else spl, page, sq, causal, cap)
  return [x.cpu() for x in got], want


def _assert_plan(got, want, table, cu):
  names = ("cu_q_prefix", "prefix_lens", "prefix_table", "suffix_table", "suffix_lens")
  rows = [r.tolist() for r in table.cpu()]
  for name, a, b in zip(names, got, want):
    assert a.dtype == torch.int32 and a.shape == b.shape, name
    if name == "prefix_table":
      for g in range(len(cu) - 1):
        if cu[g] == cu[g + 1]:
          assert a[g].tolist() in rows, f"prefix_table[{g}] (an empty group) is no row of the block table"
        else:
          assert torch.equal(a[g], b[g]), (name, g)
    else:
      assert torch.equal(a, b), (name, a.tolist(), b.tolist())


def _i32(v):
  return torch.tensor(v, dtype=torch.int32, device="cuda")


def _some_table(B, W, seed=0):
  return torch.randint(0, 5000, (B, W), generator=torch.Generator().manual_seed(seed), dtype=torch.int32).cuda()


@pytest.mark.parametrize("page", [64, 128])
@pytest.mark.parametrize("layout", ["plain", "wide_slice", "transposed"])
def test_plan_of_one_group(hip, page, layout):
  W = 6
  cap = W * page
  table = R.lay_out_table(_some_table(5, W), layout)
  lens = _i32([4 * page + 9, 3 * page, 5 * page + 1, 2 * page + 70, cap])
  # a page multiple every sequence holds; no page multiple (rounded down); above the shortest sequence (cut back, then rounded); nothing; the whole capacity
  for stated in (2 * page, 2 * page + 63, page + 1, 5 * page, 0, 10 * cap):
    for sq, causal in ((1, False), (4, True), (4, False)):
      for spl in (stated, _i32([stated])):
        got, want = _plan_both(lens, table, None, spl, page, sq, causal, cap)
        _assert_plan(got, want, table, [0, 5])
  # causal Sq 4: the shortest sequence holds exactly 2 pages + 3 - 1 keys: its first token sees 2 pages - 1 keys, so ONE page is shared, and two without causal
  lens2 = _i32([4 * page, 2 * page + 2, 3 * page])
  got, want = _plan_both(lens2, table[:3], None, 2 * page, page, 4, True, cap)
  _assert_plan(got, want, table[:3], [0, 3])
  assert got[1].tolist() == [page] and got[0].tolist() == [0, 12] and got[4].tolist() == [3 * page, page + 2, 2 * page]
  got, _ = _plan_both(lens2, table[:3], None, 2 * page, page, 4, False, cap)
  assert got[1].tolist() == [2 * page]


def test_plan_of_groups_with_an_empty_one_and_lengths_outside_the_cache(hip):
  page, W = 64, 5
  cap = W * page
  table = R.lay_out_table(_some_table(6, W, seed=1), "wide_slice")
  lens = _i32([256, 400, -5, 70, 200, 321])  # (400 and 321 exceed the capacity 320: clamped; -5 holds nothing)
  for cu in ([0, 2, 2, 3, 6], [0, 0, 6, 6], [0, 1, 2, 3, 4, 5, 6], [0, 6, 6]):
    G = len(cu) - 1
    for spl in (128, _i32([1000, 64, 64, 100, 7, 130][:G])):
      for sq, causal in ((1, False), (3, True)):
        got, want = _plan_both(lens, table, _i32(cu), spl, page, sq, causal, cap)
        _assert_plan(got, want, table, cu)
  got, _ = _plan_both(lens, table, _i32([0, 2, 2, 3, 6]), _i32([1000, 64, 64, 100]), page, 2, False, cap)
  assert got[1].tolist() == [256, 0, 0, 64] and got[0].tolist() == [0, 4, 4, 6, 12] and got[4].tolist() == [0, 64, 0, 6, 136, 256]
  # a shift past the table's width: every column of the suffix row is the row's last page
  assert got[3][0].tolist() == [int(table[0, 4])] * 5


def test_plan_of_more_sequences_and_pages_than_a_workgroup_has_lanes(hip):
  """Groups of 1, 64, 65 and 130 sequences and 67 pages per sequence: the minimum loop and the row copies take more than one trip of 64 lanes."""
  page, W, B = 64, 67, 260
  cap = W * page
  table = _some_table(B, W, seed=2)
  g = torch.Generator().manual_seed(3)
  lens = torch.randint(30 * page, cap + 200, (B,), generator=g, dtype=torch.int32)
  lens[64], lens[129], lens[259] = 7 * page + 5, 3 * page + 1, 66 * page
  cu = [0, 1, 65, 130, 260]
  got, want = _plan_both(lens.cuda(), table, _i32(cu), _i32([cap, cap, 65 * page, cap]), page, 2, True, cap)
  _assert_plan(got, want, table, cu)
  assert got[1].tolist()[1:3] == [7 * page, 3 * page]


# ---- attention
ACCURACY = [
  # page, hq, sq, causal, dtype, groups
  (64, 16, 1, False, torch.bfloat16, False),
  (64, 16, 3, True, torch.float16, True),
  (64, 128, 1, False, torch.float16, True),
  (64, 128, 3, True, torch.bfloat16, False),
  (128, 16, 3, False, torch.bfloat16, True),
  (128, 16, 1, True, torch.float16, False),
  (128, 128, 3, True, torch.float16, True),
  (128, 128, 1, False, torch.bfloat16, False),
]


def _shared_case(page, hq, sq, dtype, groups, seed, **kw):
  """One group of 6 sequences sharing 256 keys, or three groups (3, 0, 3) sharing 128 / - / 256 keys; suffixes 0, 1, Sq, 70, 129, 200."""
  suf = _suffixes(sq, 6)
  if groups:
    sizes, share = [3, 0, 3], [128, 0, 256]
    lens = [128 + s for s in suf[:3]] + [256 + s for s in suf[3:]]
  else:
    sizes, share = [6], [256]
    lens = [256 + s for s in suf]
  return _case(sizes, share, lens, hq, dtype, page, seed, sq=sq, **kw), share


@pytest.mark.parametrize("page, hq, sq, causal, dtype, groups", ACCURACY)
def test_cascade_against_float64_and_the_plain_call(hip, page, hq, sq, causal, dtype, groups):
  from ffpa_attn_amd import ffpa_attn_with_kvcache_mla, ffpa_attn_with_kvcache_mla_cascade

  t, share = _shared_case(page, hq, sq, dtype, groups, seed=page + hq + sq)
  kw = dict(cache_seqlens=t["lens"], block_table=t["table"], softmax_scale=SCALE, causal=causal, return_softmax_lse=True)
  spl = _i32(share) if groups else share[0]
  cas, lse_c = ffpa_attn_with_kvcache_mla_cascade(t["q"], t["pool"], DV, shared_prefix_len=spl, cu_group_seqs=t["cu_t"] if groups else None,
                                                  max_group_seqs=3 if groups else None, cascade=True, **kw)
  plain, _ = ffpa_attn_with_kvcache_mla(t["q"], t["pool"], DV, **kw)
  torch.cuda.synchronize()
  assert cas.shape == (6, sq, hq, DV) and cas.dtype == dtype and lse_c.shape == (6, hq, sq) and lse_c.dtype == torch.float32
  ref, ref_lse = _float64(t, causal)
  _check_accuracy(cas, lse_c, plain, ref, ref_lse, dtype)
  # the prefix really was split off: the plan of this call has the shared pages in it (under causal Sq 3 the sequence without a suffix cuts a page off)
  got = torch.ops.ffpa_attn._mla_cascade_plan_hip(t["lens"], t["table"], t["cu_t"] if groups else None, spl if groups else None, 0 if groups else spl, page, sq,
                                                  1 if causal else 0, t["cap"])
  cut = page if causal and sq > 1 else 0  # (the sequence without a suffix holds exactly the shared keys: its first causal token sees Sq - 1 fewer)
  want = [share[0] - cut, 0, share[2]] if groups else [share[0] - cut]  # (of three groups the first holds that sequence, the last does not)
  assert got[1].tolist() == want


@pytest.mark.parametrize("page, hq, sq, dtype", [(64, 16, 3, torch.bfloat16), (128, 128, 1, torch.float16)])
def test_a_zero_prefix_and_cascade_false_are_the_plain_call_bit_for_bit(hip, page, hq, sq, dtype):
  from ffpa_attn_amd import ffpa_attn_with_kvcache_mla, ffpa_attn_with_kvcache_mla_cascade

  t, share = _shared_case(page, hq, sq, dtype, True, seed=5, nan_unused=False, extra_pages=1)
  kw = dict(cache_seqlens=t["lens"], block_table=t["table"], softmax_scale=SCALE, causal=True, return_softmax_lse=True)
  plain, lse = ffpa_attn_with_kvcache_mla(t["q"], t["pool"], DV, **kw)
  for spl, mode in ((0, True), (_i32([0, 0, 0]), True), (_i32([0, 0, 0]), None), (_i32(share), False), (128, False), (0, None)):
    o, l = ffpa_attn_with_kvcache_mla_cascade(t["q"], t["pool"], DV, shared_prefix_len=spl, cu_group_seqs=t["cu_t"], cascade=mode, **kw)
    assert torch.equal(o, plain) and torch.equal(l, lse), (spl, mode)
  # cascade=False with kv= (the new rows land in the sequences' own pages): the plain call's append, the plain call's cache bytes
  new = (torch.randn((6, sq, 1, D), device="cuda") * 0.5).to(dtype)
  pool_a, pool_b = t["pool"].clone(), t["pool"].clone()
  o_a, l_a = ffpa_attn_with_kvcache_mla_cascade(t["q"], pool_a, DV, shared_prefix_len=_i32(share), cu_group_seqs=t["cu_t"], kv=new, cascade=False, **kw)
  o_b, l_b = ffpa_attn_with_kvcache_mla(t["q"], pool_b, DV, kv=new, **kw)
  assert torch.equal(o_a, o_b) and torch.equal(l_a, l_b) and torch.equal(pool_a.view(torch.int16), pool_b.view(torch.int16))
  assert not torch.equal(pool_a.view(torch.int16), t["pool"].view(torch.int16))


@pytest.mark.parametrize("page, hq, sq, causal, dtype", [(64, 16, 1, False, torch.float16), (128, 128, 3, True, torch.bfloat16)])
def test_the_prefix_is_read_through_the_first_sequence_of_every_group_only(hip, page, hq, sq, causal, dtype):
  """Every sequence but its group's first points at pages of OTHER content in its prefix columns, and pages nobody may read hold NaN: the cascade follows the
  first sequence's row.  The plain call on the table that says so (every prefix column taken from the first sequence) is the baseline of the accuracy rule."""
  from ffpa_attn_amd import ffpa_attn_with_kvcache_mla, ffpa_attn_with_kvcache_mla_cascade

  # (every suffix holds the query tokens, so the whole stated prefix is taken under causal too: the pages that differ are the pages the prefix pass serves)
  share, suf = [128, 0, 256], [sq, 70, 129, 200, sq, 129]
  t = _case([3, 0, 3], share, [128 + x for x in suf[:3]] + [256 + x for x in suf[3:]], hq, dtype, page, seed=9, sq=sq, diverge=True)
  assert not torch.equal(t["table"], t["truth"])
  planned = torch.ops.ffpa_attn._mla_cascade_plan_hip(t["lens"], t["table"], t["cu_t"], _i32(share), 0, page, sq, 1 if causal else 0, t["cap"])
  assert planned[1].tolist() == share
  kw = dict(cache_seqlens=t["lens"], softmax_scale=SCALE, causal=causal, return_softmax_lse=True)
  cas, lse_c = ffpa_attn_with_kvcache_mla_cascade(t["q"], t["pool"], DV, shared_prefix_len=_i32(share), cu_group_seqs=t["cu_t"], block_table=t["table"], cascade=True, **kw)
  plain, _ = ffpa_attn_with_kvcache_mla(t["q"], t["pool"], DV, block_table=t["truth"], **kw)
  wrong, _ = ffpa_attn_with_kvcache_mla(t["q"], t["pool"], DV, block_table=t["table"], **kw)
  torch.cuda.synchronize()
  ref, ref_lse = _float64(t, causal)
  _check_accuracy(cas, lse_c, plain, ref, ref_lse, dtype)
  assert (wrong.double() - ref).abs().max() > 50 * (plain.double() - ref).abs().max()  # (the other content is other: reading it is far off)


@pytest.mark.parametrize("page, hq, sq, causal, dtype", [(64, 128, 1, False, torch.bfloat16), (128, 16, 3, True, torch.float16)])
def test_a_stated_prefix_longer_than_a_sequence_is_cut_back(hip, page, hq, sq, causal, dtype):
  """256 keys are stated (and laid out) as shared, one sequence of the group holds 150: its pages are the shared ones, it just holds fewer keys.  The effective
  prefix is what it holds, in whole pages, and the answer is still the float64 one."""
  from ffpa_attn_amd import ffpa_attn_with_kvcache_mla, ffpa_attn_with_kvcache_mla_cascade

  lens = [256 + 70, 150, 256 + 129, 256, 256 + 1]
  t = _case([5], [256], lens, hq, dtype, page, seed=21, sq=sq)
  kw = dict(cache_seqlens=t["lens"], block_table=t["table"], softmax_scale=SCALE, causal=causal, return_softmax_lse=True)
  for spl in (256, 300, _i32([10 ** 6])):
    cas, lse_c = ffpa_attn_with_kvcache_mla_cascade(t["q"], t["pool"], DV, shared_prefix_len=spl, cascade=True, **kw)
    plain, _ = ffpa_attn_with_kvcache_mla(t["q"], t["pool"], DV, **kw)
    torch.cuda.synchronize()
    ref, ref_lse = _float64(t, causal)
    _check_accuracy(cas, lse_c, plain, ref, ref_lse, dtype)
  got = torch.ops.ffpa_attn._mla_cascade_plan_hip(t["lens"], t["table"], None, None, 256, page, sq, 1 if causal else 0, t["cap"])
  assert got[1].tolist() == [(150 - (sq - 1 if causal else 0)) // page * page]


@pytest.mark.parametrize("page, hq, sq, snew, dtype", [(64, 16, 3, 3, torch.bfloat16), (128, 128, 1, 1, torch.float16), (64, 16, 1, 2, torch.float16)])
def test_the_append_writes_the_plain_calls_bytes(hip, page, hq, sq, snew, dtype):
  from ffpa_attn_amd import ffpa_attn_with_kvcache_mla, ffpa_attn_with_kvcache_mla_cascade

  # groups of 3, 1 and 2 sequences sharing 128 / - / 256 keys
  share = [128, 0, 256]
  t = _case([3, 1, 2], share, [128, 128 + 1, 128 + sq, 70, 256 + 129, 256 + 200], hq, dtype, page, seed=31, sq=sq, nan_unused=False, extra_pages=1)
  before = t["lens"].clone()
  before[1] = t["cap"] - 1  # (one sequence runs into the capacity: its rows past it are dropped, its length is the capacity)
  before[3] = -4            # (... and a negative length appends at 0: the sequence of the group that shares nothing)
  new = (torch.randn((6, snew, 1, D), device="cuda") * 0.5).to(dtype)
  pool_c, pool_p = t["pool"].clone(), t["pool"].clone()
  kw = dict(cache_seqlens=before, block_table=t["table"], softmax_scale=SCALE, causal=True, return_softmax_lse=True, kv=new)
  spl = _i32(share)
  cas, lse_c = ffpa_attn_with_kvcache_mla_cascade(t["q"], pool_c, DV, shared_prefix_len=spl, cu_group_seqs=t["cu_t"], cascade=True, **kw)
  plain, _ = ffpa_attn_with_kvcache_mla(t["q"], pool_p, DV, **kw)
  torch.cuda.synchronize()
  assert torch.equal(pool_c.view(torch.int16), pool_p.view(torch.int16)) and not torch.equal(pool_c.view(torch.int16), t["pool"].view(torch.int16))
  assert torch.equal(before, _i32(before.tolist()))
  after = [min(max(n, 0) + snew, t["cap"]) for n in before.tolist()]
  ref, ref_lse = _float64(t, True, lens=after, pool=pool_p)
  _check_accuracy(cas, lse_c, plain, ref, ref_lse, dtype)
  got = torch.ops.ffpa_attn._mla_cascade_plan_hip(_i32(after), t["table"], t["cu_t"], spl, 0, page, sq, 1, t["cap"])
  assert got[1].tolist() == share


@pytest.mark.parametrize("page, hq, sq, causal, dtype", [(64, 16, 3, True, torch.bfloat16), (128, 128, 1, False, torch.float16)])
def test_fp8(hip, page, hq, sq, causal, dtype):
  from ffpa_attn_amd import (ffpa_attn_with_kvcache_mla_cascade, ffpa_attn_with_kvcache_mla_cascade_fp8, ffpa_attn_with_kvcache_mla_fp8, quantize_latent_rows)

  t, share = _shared_case(page, hq, sq, dtype, True, seed=41, extra_pages=1)
  spl = _i32(share)
  kw = dict(shared_prefix_len=spl, cu_group_seqs=t["cu_t"], cache_seqlens=t["lens"], block_table=t["table"], causal=causal, return_softmax_lse=True, cascade=True)
  # a power-of-two scale: the bits of the 16-bit cascade on the dequantised pool
  for kv_scale in (1.0, 0.25):
    pool8 = quantize_latent_rows(t["pool"], kv_scale)
    o8, l8 = ffpa_attn_with_kvcache_mla_cascade_fp8(t["q"], pool8, DV, kv_scale=kv_scale, softmax_scale=SCALE, **kw)
    o16, l16 = ffpa_attn_with_kvcache_mla_cascade(t["q"], pool8.to(dtype), DV, softmax_scale=SCALE * kv_scale, **kw)
    torch.cuda.synchronize()
    assert not torch.isnan(o8).any()
    # (fp16 O under a scale other than 1: fp16(kv_scale * x) is not kv_scale * fp16(x) where either is subnormal — the 16-bit side rounds before it scales; as in
    # tests/test_kvcache_mla_fp8_gpu.py, fp16 is held to the bits of O at scale 1 and to the bits of the LSE at every scale, bf16 to both at every scale)
    if dtype == torch.bfloat16 or kv_scale == 1.0:
      assert torch.equal(o8, o16 * kv_scale), kv_scale
    assert torch.equal(torch.isfinite(l8), torch.isfinite(l16)) and torch.equal(l8[torch.isfinite(l8)], l16[torch.isfinite(l16)])
  # any scale: the accuracy rule against the plain FP8 call, the reference over the dequantised codes
  pool8 = quantize_latent_rows(t["pool"], 0.37)
  cas, lse_c = ffpa_attn_with_kvcache_mla_cascade_fp8(t["q"], pool8, DV, kv_scale=0.37, softmax_scale=SCALE, **kw)
  plain, _ = ffpa_attn_with_kvcache_mla_fp8(t["q"], pool8, DV, kv_scale=0.37, cache_seqlens=t["lens"], block_table=t["table"], softmax_scale=SCALE, causal=causal,
                                            return_softmax_lse=True)
  torch.cuda.synchronize()
  ref, ref_lse = _float64(t, causal, pool=pool8.double() * 0.37)
  _check_accuracy(cas, lse_c, plain, ref, ref_lse, dtype)
  # ... and its append quantises as the plain FP8 call's does
  new = (torch.randn((6, sq, 1, D), device="cuda") * 0.5).to(dtype)
  pa, pb = pool8.clone(), pool8.clone()
  # (the new rows land behind what the sequences hold, in their own pages: two sequences appending into one shared page would be the caller's race)
  ffpa_attn_with_kvcache_mla_cascade_fp8(t["q"], pa, DV, kv_scale=0.37, softmax_scale=SCALE, kv=new, **kw)
  ffpa_attn_with_kvcache_mla_fp8(t["q"], pb, DV, kv_scale=0.37, kv=new, cache_seqlens=t["lens"], block_table=t["table"], softmax_scale=SCALE, causal=causal)
  torch.cuda.synchronize()
  assert torch.equal(pa.view(torch.uint8), pb.view(torch.uint8)) and not torch.equal(pa.view(torch.uint8), pool8.view(torch.uint8))


def test_one_hip_graph_follows_lengths_table_prefixes_and_groups_written_in_place(hip):
  from ffpa_attn_amd import ffpa_attn_with_kvcache_mla_cascade

  page, hq, sq = 64, 16, 3
  t, share = _shared_case(page, hq, sq, torch.bfloat16, True, seed=51, nan_unused=False, extra_pages=1)
  lens, table, spl, cu = t["lens"], t["table"], _i32(share), t["cu_t"]
  new = (torch.randn((6, sq, 1, D), device="cuda") * 0.5).to(torch.bfloat16)
  pool_g, pool_e = t["pool"].clone(), t["pool"].clone()
  call = lambda pool, lens, table, spl, cu: ffpa_attn_with_kvcache_mla_cascade(
    t["q"], pool, DV, shared_prefix_len=spl, cu_group_seqs=cu, max_group_seqs=6, kv=new, cache_seqlens=lens, block_table=table, softmax_scale=SCALE, causal=True,
    return_softmax_lse=True, cascade=True)
  side = torch.cuda.Stream()
  side.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(side):
    call(pool_g.clone(), lens, table, spl, cu)
  torch.cuda.current_stream().wait_stream(side)
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    out, lse = call(pool_g, lens, table, spl, cu)
  # (groups of 3, 0, 3 sharing 128 / - / 256 keys; then 2, 2, 2: the middle group's sequences share nothing, which its stated 0 says; then one group of 6 ...)
  steps = [None, ([0, 2, 4, 6], [128, 0, 256], 1), ([0, 0, 3, 6], [999, 64, 200], 2), ([0, 3, 3, 6], [0, 0, 0], 0)]
  for step in steps:
    if step is not None:
      cu.copy_(_i32(step[0]))
      spl.copy_(_i32(step[1]))
      lens.add_(step[2])
      own = table[:, 4:].clone()
      table[:, 4:] = own.roll(1, dims=1)  # (the sequences' own pages in another order: other keys behind the shared ones)
    graph.replay()
    eo, el = call(pool_e, lens.clone(), table.clone(), spl.clone(), cu.clone())
    torch.cuda.synchronize()
    assert torch.equal(out, eo) and torch.equal(lse, el), step
    assert torch.equal(pool_g.view(torch.int16), pool_e.view(torch.int16)), step
    assert not torch.isnan(out).any()


def test_torch_compile_and_opcheck(hip):
  from ffpa_attn_amd import ffpa_attn_with_kvcache_mla_cascade

  t, share = _shared_case(64, 16, 3, torch.float16, True, seed=61, nan_unused=False)
  spl = _i32(share)

  def f(q, pool, lens, table, spl, cu):
    return ffpa_attn_with_kvcache_mla_cascade(q, pool, DV, shared_prefix_len=spl, cu_group_seqs=cu, cache_seqlens=lens, block_table=table, softmax_scale=SCALE,
                                              causal=True, cascade=True) * 2

  args = (t["q"], t["pool"], t["lens"], t["table"], spl, t["cu_t"])
  eager = f(*args)
  compiled = torch.compile(f)(*args)
  torch.cuda.synchronize()
  assert torch.equal(eager, compiled)
  torch.library.opcheck(torch.ops.ffpa_attn._mla_cascade_plan_hip.default, (t["lens"], t["table"], t["cu_t"], spl, 0, 64, 3, 1, t["cap"]))
  torch.library.opcheck(torch.ops.ffpa_attn._mla_cascade_plan_hip.default, (t["lens"], t["table"], None, None, 128, 64, 1, 0, t["cap"]))
