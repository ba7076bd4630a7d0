"""The thirteen MLA latent-cache calls on the GPU against ONE float64 reference (tests/kvcache_mla_family_ref.py), over the seeded family sweep: every case is
materialised on the GPU, its call runs once under the launch flags the case names (forced KV ranges, the non-temporal fetch forced on or off), and O and LSE are
held to ``kvcache_ref.check`` UNCHANGED — no tolerance of this file's own.  Where the case appends (``kv=``, or ``store_latent_rows_ds`` in front of the
656-byte-row call), the pool's WHOLE storage must equal the reference's byte for byte: copies in a 16-bit pool, ``quantize_latent_rows`` in an FP8 pool,
``pack_latent_rows_ds`` in a pool of 656-byte rows — and without an append it must be untouched.  Every byte no sequence reads is NaN, so a finite output says no
unused page, guard row or entry behind a count was read.  The plan of every launch (``plan_out``) must name the build the case asks for.  The generator's
coverage is asserted on the CPU (tests/test_kvcache_mla_family.py)."""

import contextlib

import pytest
import torch

import kvcache_mla_family_ref as F
import kvcache_ref as R
from test_fwd_gpu import hip  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def _launches(hip, flags=0):
  """Every latent launch inside the block — dense or sparse — carries ``flags`` too, and its plan (``plan_out``) is appended to the list the block receives."""
  plans, real = [], (hip.mla_forward, hip.mla_sparse_forward)

  def spy_on(fn):
    def spy(*args, **kw):
      plan = {}
      kw["flags"] = kw.get("flags", 0) | flags
      kw["plan_out"] = plan
      out = fn(*args, **kw)
      plans.append(plan)
      return out
    return spy

  hip.mla_forward, hip.mla_sparse_forward = spy_on(real[0]), spy_on(real[1])
  try:
    yield plans
  finally:
    hip.mla_forward, hip.mla_sparse_forward = real


def _flags(hip, c) -> int:
  stream = {"auto": 0, "on": hip.FLAG_KV_STREAM, "off": hip.FLAG_NO_KV_STREAM}[c["stream"]]
  return stream | (hip.FLAG_FORCE_SPLITS if c["num_splits"] > 1 else 0)


def _run(c, t):
  """The case's call, by its public name."""
  import ffpa_attn_amd

  fn = getattr(ffpa_attn_amd, c["call"])
  kw = dict(softmax_scale=c["scale"], num_splits=c["num_splits"], return_softmax_lse=True)
  if c["fp8"]:
    kw["kv_scale"] = c["kv_scale"]
  if c["sparse"]:
    if c["append"] == "store":
      ffpa_attn_amd.store_latent_rows_ds(t["kv_cache"], t["store_kv"], t["store_slots"])
    return fn(t["q"], t["kv_cache"], F.DV, t["indices"], topk_lens=t["topk_lens"], **kw)
  if c["tree"]:
    kw["tree_mask"] = t["tree_mask"]
  else:
    kw["causal"] = c["causal"]
  if t["kv"] is not None:
    kw["kv"] = t["kv"]
  if c["cascade"]:
    kw.update(shared_prefix_len=t["shared_prefix_len"], cu_group_seqs=t["cu_group_seqs"], max_group_seqs=t["max_group_seqs"], cascade=True)
  if c["ragged"]:
    return fn(t["q"], t["kv_cache"], F.DV, t["cu_seqlens_q"], c["Sq"], t["lens"], t["table"], **kw)
  return fn(t["q"], t["kv_cache"], F.DV, cache_seqlens=t["lens"], block_table=t["table"], **kw)


def _bits(x):
  return x.view(torch.int16) if x.element_size() == 2 else x


@pytest.mark.parametrize("seed", F.SWEEP_SEEDS)
def test_mla_family_sweep(hip, seed):
  c = F.draw_case(seed)
  t = F.materialize(c, "cuda")
  before = t["storage"].clone()
  ref, vstat, want_storage = F.reference(c, t)  # (float64 on the GPU, on a clone of the storage: the call below appends in place)
  with _launches(hip, _flags(hip, c)) as plans:
    out, lse = _run(c, t)
  torch.cuda.synchronize()
  hq, T = c["heads"][0], sum(c["qlens"])
  what = f"seed {seed} {c['call']} {c['dtype']} heads {c['heads']} tokens {c['qlens'] if c['ragged'] else (c['B'], c['Sq']) if not c['sparse'] else c['T']}"
  # the launches: the build the case names, its non-temporal choice, its forced ranges (down to one 32-key tile per range)
  assert len(plans) == (2 if c["cascade"] else 1), (what, plans)
  for plan in plans:
    assert plan["kernel"].startswith(F.kernel_of(c)), (what, plan)
    if c["stream"] != "auto":
      assert (", NT>" in plan["kernel"]) == (c["stream"] == "on"), (what, plan)
    if c["num_splits"]:
      assert plan["splits"] == min(c["num_splits"], -(-c["capacity"] // 32)), (what, plan)
    assert ("ffpa_varlen_merge_kernel" in plan["kernel"]) == (plan["splits"] > 1), (what, plan)
  # shapes, then O and LSE against float64
  if c["ragged"] or c["sparse"]:
    assert out.shape == (T, hq, F.DV) and lse.shape == (hq, T), what
  else:
    assert out.shape == (c["B"], c["Sq"], hq, F.DV) and lse.shape == (c["B"], hq, c["Sq"]), what
  assert out.dtype == R.TORCH_DTYPE[c["dtype"]] and lse.dtype == torch.float32, what
  o, l = F.flat(c, out, lse)
  assert torch.isfinite(o).all() and not torch.isnan(l).any(), f"{what}: a NaN page, guard row or tail entry was read"
  empty = torch.isneginf(ref[1])
  assert (o.transpose(1, 2)[empty] == 0).all() and torch.isneginf(l[empty]).all() and torch.isfinite(l[~empty]).all(), what
  ratio = R.check(o, l, ref, v=vstat, dtype=c["dtype"], name=what)
  print(f"\nfamily sweep: {what} splits {c['num_splits']} append {c['append']} keys {c['capacity']}: worst error / allowance {ratio:.3f}")
  # the pool: the reference's storage, byte for byte — the appended rows in the pool's format, everything else as it was
  assert torch.equal(_bits(t["storage"]), _bits(want_storage)), f"{what}: {int((_bits(t['storage']) != _bits(want_storage)).sum())} elements of the pool's storage differ"
  if c["append"] == "none":
    assert torch.equal(_bits(t["storage"]), _bits(before)), what
