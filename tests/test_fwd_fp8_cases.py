"""The exact cases of the FP8 forward's GPU tests (tests/fwd_fp8_cases.py), checked without a GPU: for EVERY case a GPU test runs, the conditions under
which the kernel's arithmetic is exact, scales that differ wherever an index could be dropped, a reference that moves in the output dtype when a row's limit
moves by one key either way, and carriers that together stand on every lane position of the V8T permutation."""

import pytest
import torch

import fwd_fp8_cases as fc
from ffpa_attn_amd.interface import FP8_BLOCK_KEYS as K

CASES = fc.all_gpu_cases()
# the shapes the construction was first tried on (D = 256, B = 1, Hq = Hkv = 2, causal), and the same under GQA with four heads per KV head
TRIED = [(63, 127), (64, 128), (65, 129), (128, 128), (129, 257), (64, 256), (1, 128), (1, 129), (127, 255), (192, 128), (130, 64)]
EXTRA = [(1, 2, 2, nq, nkv, 256, True) for nq, nkv in TRIED] + [(1, 8, 2, nq, nkv, 256, True) for nq, nkv in TRIED]


def _id(args):
  B, hq, hkv, nq, nkv, D, causal = args
  return f"B{B}-Hq{hq}-Hkv{hkv}-{nq}x{nkv}-D{D}-{'causal' if causal else 'full'}"


@pytest.mark.parametrize("args", CASES + [a for a in EXTRA if a not in CASES], ids=_id)
def test_case_is_exact_varied_and_sharp(args):
  c = fc.exact_case(*args)  # (conditions 1 and 2 are asserted by the builder; here once more, on scores of an independent reference)
  B, hq, hkv, nq, nkv, D, causal = args
  want, p, live, s = fc.attend2(*fc.dequantised(c), causal)
  fc.assert_exact_conditions(c, s)
  # the builder's reference is attend2's, bit for bit, and a row has a key exactly where its limit says so
  assert torch.equal(torch.where(live, want, torch.zeros_like(want)), c.want) and torch.equal(live, c.live)
  assert torch.equal(live[0, 0, :, 0], c.limits >= 0) and bool((c.want[~live.expand_as(want)] == 0).all())
  # the carrier is the row's last visible key and holds +1 on the row's column: its score is +1 x the two scales, the largest a key of its tile can have
  limits = fc.row_limits(nq, nkv, causal)
  assert torch.equal(c.limits, limits) and int(limits.max()) == nkv - 1
  for b in range(B):
    for h in range(hq):
      has = limits >= 0
      cols = c.qc[b, h, has].argmax(-1)
      assert bool((c.kc[b, h // (hq // hkv), limits[has], cols] == 1).all())
      assert bool((s[b, h, has, limits[has]] == (c.q_scale[b, h].repeat_interleave(fc.R)[:nq] * c.k_scale[b, h // (hq // hkv)].repeat_interleave(K)[:nkv][limits.clamp(min=0)])[has]).all())
  # condition 3, in both output dtypes
  for name, dtype in fc.DTYPES.items():
    blind = fc.mutation_blind_rows(c, dtype)
    assert blind[+1] == 0 and blind[-1] == 0, (c.name, name, blind)
    assert blind["rows -1"] == int((limits >= 0).sum()) and blind["rows +1"] == int(((limits >= -1) & (limits < nkv - 1)).sum())


@pytest.mark.parametrize("group", ["every build", "seams D256", "seams D448"])
def test_carriers_cover_every_lane_position(group):
  """Condition 4: over one parametrised group of cases the carriers stand on every ``key % 128`` — every position of the V8T permutation, and (both halves
  of a tile being carried) every 16-byte piece a lane reads."""
  if group == "every build":
    cases = [a for _, a in fc.every_build_cases()]
  else:
    cases = [a for gid, g in fc.seam_groups().items() if gid.startswith(group.split()[1] + "-") for a in g]
  lanes = set()
  for args in cases:
    carrier = fc.exact_case(*args).carrier
    lanes |= set((carrier[carrier >= 0] % K).unique().tolist())
  # (the two shapes of "every build" carry keys 190 ... 258 and 0 ... 60: every position but 61, which the seam groups hold)
  assert lanes == set(range(K)) - ({61} if group == "every build" else set()), sorted(set(range(K)) - lanes)


def test_scales_differ_along_every_axis():
  """Condition 2 as the kernel's indices need it: ``qtile = (b Hq + hq) RT + rt`` and ``kvhead NT + t`` — a scale read with any one of the three indices
  dropped is another number somewhere."""
  for args in CASES:
    c = fc.exact_case(*args)
    for t in (c.q_scale, c.k_scale):
      for axis in range(3):
        n = t.size(axis)
        assert n == 1 or bool((t.narrow(axis, 0, n - 1) != t.narrow(axis, 1, n - 1)).any()), (c.name, axis)


def test_a_wrong_scale_index_or_limit_shows():
  """The tests' own sanity, on the reference: the mutations a kernel could carry move the expected BITS of one case — q_scale read by row tile alone, k_scale
  of the first tile everywhere, ``>=`` for ``>`` at the limit (one key fewer), a key tile dropped (``nt`` without its + 1)."""
  c = fc.exact_case(2, 8, 2, 69, 259, 448, True)
  true = fc.expected(c, torch.bfloat16)

  def moved(limits=c.limits, **scales):
    return fc.expected(c._replace(want=fc.attend_limits(c._replace(**scales), limits)[0]), torch.bfloat16)

  assert not torch.equal(moved(q_scale=c.q_scale[:1, :1].expand_as(c.q_scale).contiguous()), true)
  assert not torch.equal(moved(k_scale=c.k_scale[..., :1].expand_as(c.k_scale).contiguous()), true)
  assert not torch.equal(moved(limits=c.limits - 1), true)
  assert not torch.equal(moved(limits=torch.minimum(c.limits, (c.limits // K) * K - 1)), true)
