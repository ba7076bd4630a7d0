"""The fragment read-ahead of the single-tile MFMA loops (csrc/ffpa_fwd_m16_tile.inc, FFPA_M16_GAP_SPLIT): a V^T fragment is requested as two transpose reads
that sit in different MFMA gaps, a K fragment's read may sit between the MFMAs of the fragment in front of it.

What can go wrong there is a fragment assembled from the wrong halves, read from the wrong column block or key half, or not requested at all at the loop's edges
(the last PF2 / PF1 fragments request nothing; the address tables VV / KV differ between D % 128 == 0 and == 64).  So: every head dim class, one KV tile, one tile
and a key, three tiles less a key, one row tile and a ragged second one, plain and causal, through the public calls — against a float64 softmax . V under the
allowances of tests/test_m16_lane_growth_gpu.py (imported, as tests/test_kvcache_family_gpu.py does), and once per dtype with V = +-(column - D / 2): distinct
integers that the 16-bit formats hold exactly, the sign by the 16-key half of a fragment, so that a wrong column block or key half is an error of whole units.
"""

import functools

import pytest
import torch

from test_fwd_gpu import hip  # noqa: F401  (fixture)
from test_m16_lane_growth_gpu import TOL, _assert_close, _ref64

pytestmark = pytest.mark.gpu

H = 2
DIMS = (128, 192, 256, 320, 448, 512, 576, 640)
DTYPES = [torch.bfloat16, torch.float16]


@functools.lru_cache(maxsize=None)
def _case(D, dtype, nq, nkv):
  """Q, K, V ~ N(0, 1) and the float64 results without and with the (tail-aligned) causal mask: computed once per shape, never written to."""
  g = torch.Generator(device="cuda").manual_seed(3000 + D + 7 * nq + nkv)
  q = torch.randn((1, H, nq, D), dtype=dtype, device="cuda", generator=g)
  k = torch.randn((1, H, nkv, D), dtype=dtype, device="cuda", generator=g)
  v = torch.randn((1, H, nkv, D), dtype=dtype, device="cuda", generator=g)
  vis = (torch.arange(nkv, device="cuda")[None, :] <= torch.arange(nq, device="cuda")[:, None] + (nkv - nq))[None, None]
  return q, k, v, _ref64(q, k, v, D ** -0.5), _ref64(q, k, v, D ** -0.5, visible=vis)


def _nkvs(hip, D):
  bc = hip.tile_config(D)["block_keys"]
  return {"one_tile": bc, "one_tile_and_a_key": bc + 1, "three_tiles_less_a_key": 3 * bc - 1}


@pytest.mark.parametrize("causal", [False, True], ids=["plain", "causal"])
@pytest.mark.parametrize("keys", ["one_tile", "one_tile_and_a_key", "three_tiles_less_a_key"])
@pytest.mark.parametrize("nq", [32, 129])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
@pytest.mark.parametrize("D", DIMS)
def test_dense_call(hip, D, dtype, nq, keys, causal):
  nkv = _nkvs(hip, D)[keys]
  q, k, v, plain, masked = _case(D, dtype, nq, nkv)
  o, lse = hip.forward(q, k, v, None, causal, D ** -0.5, num_splits=1)
  o_ref, lse_ref = masked if causal else plain
  _assert_close(o, lse, o_ref, lse_ref, dtype, f"D{D} {dtype} Nq{nq} Nkv{nkv} causal={causal}")


def _integer_v(nkv, D, dtype):
  """V[key, d] = +-(d - D / 2): whole numbers of magnitude <= 256 for D <= 512 (exact in bf16 and fp16), distinct over the columns; the sign flips with the
  16-key half of a 32-key fragment."""
  col = torch.arange(D, device="cuda", dtype=torch.float32) - D // 2
  sign = 1.0 - 2.0 * ((torch.arange(nkv, device="cuda") // 16) % 2).float()
  v = (sign[:, None] * col[None, :]).to(dtype)
  assert torch.equal(v.float(), sign[:, None] * col[None, :])
  return v[None, None].expand(1, H, nkv, D).contiguous()


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16"])
def test_integer_valued_v_columns(hip, dtype):
  """D = 512, 129 rows over three tiles less a key.  O[d] = (d - 256) w, w = the row's softmax weight on the even 16-key halves minus that on the odd ones.
  Every query row and every key of an even half carry 8 u (u a fixed unit vector) on top of N(0, 1): + 64 / sqrt(512) = 2.8 on those scores, so w is
  large on every row (asserted on the float64 result: >= 0.5).  A fragment from the neighbouring column block is then off by 16 w >= 8 at every column and one with
  its key halves swapped by 2 |O|, against an allowance of TOL (1 + |O|) <= TOL (1 + 256): nothing for rounding to hide."""
  D, nq = 512, 129
  nkv = _nkvs(hip, D)["three_tiles_less_a_key"]
  g = torch.Generator(device="cuda").manual_seed(4000)
  u = torch.randn(D, device="cuda", generator=g)
  u = 8.0 * u / u.norm()
  even = ((torch.arange(nkv, device="cuda") // 16) % 2 == 0).float()
  q = (torch.randn((1, H, nq, D), device="cuda", generator=g) + u).to(dtype)
  k = (torch.randn((1, H, nkv, D), device="cuda", generator=g) + even[:, None] * u).to(dtype)
  v = _integer_v(nkv, D, dtype)
  o, lse = hip.forward(q, k, v, None, False, D ** -0.5, num_splits=1)
  o_ref, lse_ref = _ref64(q, k, v, D ** -0.5)
  w = o_ref[..., D // 2 + 100] / 100.0
  assert w.min().item() >= 0.5, w.min().item()
  assert 16 * w.min().item() > 1.5 * TOL[dtype] * (1 + 256) and 2 * 16 * w.min().item() > 1.5 * TOL[dtype] * (1 + 16)  # (either mistake is past the allowance)
  _assert_close(o, lse, o_ref, lse_ref, dtype, f"integer V {dtype}")


def _packed(dtype, D, nq, nkv, seed):
  g = torch.Generator(device="cuda").manual_seed(seed)
  q = torch.randn((1, H, nq, D), dtype=dtype, device="cuda", generator=g)
  k = torch.randn((1, H, nkv, D), dtype=dtype, device="cuda", generator=g)
  v = torch.randn((1, H, nkv, D), dtype=dtype, device="cuda", generator=g)
  return q, k, v


def _check_packed(o, lse, seqs, D, dtype, name):
  r0 = 0
  for i, (qs, ks, vs) in enumerate(seqs):
    n = qs.size(2)
    o_ref, lse_ref = _ref64(qs, ks, vs, D ** -0.5)
    _assert_close(o[r0:r0 + n].transpose(0, 1)[None], lse[:, r0:r0 + n][None], o_ref, lse_ref, dtype, f"{name} seq {i}")
    r0 += n


def _two_sequences(dtype, D):
  """129 rows over two 64-key tiles and 32 rows over two tiles and a key, packed."""
  seqs = (_packed(dtype, D, 129, 128, 11), _packed(dtype, D, 32, 129, 12))
  q = torch.cat([s[0][0] for s in seqs], dim=1).transpose(0, 1).contiguous()  # [T, H, D]
  k = torch.cat([s[1][0] for s in seqs], dim=1).transpose(0, 1).contiguous()
  v = torch.cat([s[2][0] for s in seqs], dim=1).transpose(0, 1).contiguous()
  cu_q = torch.tensor([0, 129, 161], dtype=torch.int32, device="cuda")
  cu_k = torch.tensor([0, 128, 257], dtype=torch.int32, device="cuda")
  return q, k, v, cu_q, cu_k, seqs


def test_packed_call(hip):
  dtype, D = torch.bfloat16, 512
  q, k, v, cu_q, cu_k, seqs = _two_sequences(dtype, D)
  plan = {}
  o, lse = hip.varlen_forward(q, k, v, cu_q, cu_k, 129, 129, False, D ** -0.5, num_splits=1, plan_out=plan)
  assert "m16_varlen" in plan["kernel"], plan
  _check_packed(o, lse, seqs, D, dtype, "packed")


def test_paged_call(hip):
  """The same two sequences, their keys in 64-key pages handed out in reverse order."""
  dtype, D = torch.bfloat16, 512
  q, k, v, cu_q, _, seqs = _two_sequences(dtype, D)
  page, ppr = 64, 3
  pk = torch.zeros(2 * ppr, page, H, D, dtype=dtype, device="cuda")
  pv = torch.zeros_like(pk)
  table = torch.arange(2 * ppr - 1, -1, -1, dtype=torch.int32, device="cuda").view(2, ppr).contiguous()
  for i, (lo, hi) in enumerate(((0, 128), (128, 257))):
    for j in range(-(-(hi - lo) // page)):
      rows = slice(lo + j * page, min(lo + (j + 1) * page, hi))
      n = rows.stop - rows.start
      pk[int(table[i, j]), :n] = k[rows]
      pv[int(table[i, j]), :n] = v[rows]
  used = torch.tensor([128, 129], dtype=torch.int32, device="cuda")
  plan = {}
  o, lse = hip.varlen_forward(q, pk, pv, cu_q, None, 129, ppr * page, False, D ** -0.5, seqused_k=used, block_table=table, num_splits=1, plan_out=plan)
  assert plan["kernel"].startswith("ffpa_fwd_m16_paged_kernel"), plan
  _check_packed(o, lse, seqs, D, dtype, "paged")


def test_mla_latent_call(hip):
  """One sequence over the latent pool (keys = the 576-wide rows, values = their first 512 columns), two 64-key tiles; 16 heads x 8 tokens = 128 rows."""
  dtype, D, DV, hq, sq, nkv = torch.bfloat16, 576, 512, 16, 8, 128
  if (D, DV) not in hip.MLA_BUILDS:
    pytest.fail(f"the MLA latent kernel is not built for ({D}, {DV})")
  g = torch.Generator(device="cuda").manual_seed(78)
  q = torch.randn((sq, hq, D), dtype=dtype, device="cuda", generator=g)
  rows = torch.randn((nkv, D), dtype=dtype, device="cuda", generator=g)
  page, ppr = 64, 2
  pool = torch.zeros(ppr, page, 1, D, dtype=dtype, device="cuda")
  table = torch.tensor([[1, 0]], dtype=torch.int32, device="cuda")
  for j in range(ppr):
    pool[int(table[0, j]), :, 0] = rows[j * page:(j + 1) * page]
  cu_q = torch.tensor([0, sq], dtype=torch.int32, device="cuda")
  used = torch.tensor([nkv], dtype=torch.int32, device="cuda")
  o, lse = hip.mla_forward(q, pool, DV, cu_q, used, table, sq, ppr * page, False, D ** -0.5, num_splits=1)
  q4 = q.transpose(0, 1)[None]  # [1, hq, sq, D]
  k4 = rows[None, None].expand(1, hq, nkv, D)
  o_ref, lse_ref = _ref64(q4, k4, k4[..., :DV], D ** -0.5)
  _assert_close(o.transpose(0, 1)[None], lse[None], o_ref, lse_ref, dtype, "mla")
