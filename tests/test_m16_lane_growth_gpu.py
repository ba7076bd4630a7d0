"""The lazy rescale's growth test of the single-tile prefill builds (D <= 512), which every lane runs on its OWN partial row maximum: the 4-lane
reduction of the row maxima only runs on the KV steps where some lane passed ``m_run + thr`` (csrc/ffpa_fwd_m16_tile.inc, "online softmax").

What can go wrong there is a row maximum that grows and is not seen — in one lane of the row's four, in one row half of one wave, in the first, a
middle, the last full or the ragged tile — or one that is seen and should not have been.  So: Q, K, V ~ N(0, 1) and a SPIKE, K[kspike] = g Q[row] / |Q[row]|,
which lifts exactly that row's score at exactly that key to ~ g (natural units; the threshold is 8 log2 units ~ 5.5), everywhere the test can reach, against
a float64 softmax . V built here (the tolerances of tests/test_fwd_gpu.py: atol = rtol = 2e-2 bf16 / 1e-2 fp16 on O, atol 3e-4 / rtol 3e-5 on the natural-log
LSE) and, where it covers the case, against the CPU oracle, which walks the same tiles with the same threshold.

Shapes: B 1, H 2, one row tile (128 rows: all four waves), Nkv = 3 BC + 5 (three full tiles and a ragged one).
"""

import math

import numpy as np
import pytest
import torch

from oracle import ffpa_oracle as fo

pytestmark = pytest.mark.gpu

TOL = {torch.bfloat16: 2e-2, torch.float16: 1e-2}  # tests/test_fwd_gpu.py: atol = rtol on O
LSE_ATOL, LSE_RTOL = 3e-4, 3e-5                    # ditto, LSE against float64
LOG2E = 1.4426950408889634
THR = 8.0      # the library's default rescale threshold, log2 units
G_FAR = 30.0   # a spike's score, natural units: 43 log2 units, far past everything N(0, 1) data and the threshold add up to
H, NQ = 2, 128
BC = {128: 64, 256: 128, 320: 128, 512: 64}


@pytest.fixture(scope="module")
def hip():
  if not torch.cuda.is_available():
    pytest.fail("these tests need a GPU; run with -m 'not gpu' on CPU boxes")
  from ffpa_attn_amd import hip as h

  h.load_library()  # fail loudly if the extension is missing: there is no fallback
  return h


def _nkv(D):
  return 3 * BC[D] + 5


# (name, [(row, tile, key inside the tile, gain or None = half a threshold above the row's maximum over tile 0)]): tile 3 is the ragged one (5 keys)
CASES = [("none", []), ("tile0", [(5, 0, 7, G_FAR)]), ("last_full_tile", [(5, 2, 7, G_FAR)]), ("ragged_tail", [(5, 3, 3, G_FAR)])]
CASES += [(f"row{r}", [(r, 1, 7, G_FAR)]) for r in (0, 15, 16, 31, 127)]       # row halves 0 / 1 of waves 0 and 3
CASES += [(f"key{c}", [(40, 1, 16 + c, G_FAR)]) for c in (0, 7, 9, 12, 15)]    # key % 16 / 4 = the lane of the row's four that holds the winner: 0, 1, 2, 3, 3
CASES += [("two_rows_one_step", [(3, 1, 7, G_FAR), (20, 1, 12, G_FAR)]), ("two_rows_two_steps", [(3, 1, 7, G_FAR), (20, 2, 12, G_FAR)]),
          ("below_threshold", [(5, 1, 7, None)])]


def _inputs(D, dtype, spikes, nkv=None, seed=0, heads=H, nq=NQ, bc=None):
  """Q, K, V ~ N(0, 1) in ``dtype`` (the same for every case of a head dim), K with the case's spikes.  Returns q, k, v and the log2-domain growth of every
  spiked row's score over the row's maximum over the other keys of tile 0.  ``bc``: the KV tile the spikes are laid out for (default: the dense launch's
  ``BC[D]``; the paged builds walk 64-key tiles at every D <= 512: tests/test_kvcache_family_gpu.py)."""
  bc = bc or BC[D]
  nkv = nkv or 3 * bc + 5
  g = torch.Generator(device="cuda").manual_seed(1000 + D + seed)
  q = torch.randn((1, heads, nq, D), dtype=dtype, device="cuda", generator=g)
  k = torch.randn((1, heads, nkv, D), dtype=dtype, device="cuda", generator=g)
  v = torch.randn((1, heads, nkv, D), dtype=dtype, device="cuda", generator=g)
  grown = []
  for row, tile, col, gain in spikes:
    key = tile * bc + col
    assert key < nkv
    qr = q[0, :, row].double()
    norm = qr.norm(dim=-1, keepdim=True)
    if gain is None:
      # the row's running maximum behind tile 0 (natural units) + half a threshold: grows, and must not rescale
      m0 = (qr[:, None, :] * k[0, :, :bc].double()).sum(-1).max(dim=-1).values * D ** -0.5
      gain_h = (m0 + 0.5 * THR / LOG2E)[:, None]
    else:
      gain_h = torch.full_like(norm, gain)
    k[0, :, key] = (gain_h * math.sqrt(D) * qr / (norm * norm)).to(dtype)  # score = scale q.k = gain
    s_new = (qr * k[0, :, key].double()).sum(-1) * D ** -0.5
    s_old = (qr[:, None, :] * k[0, :, :bc].double()).sum(-1) * D ** -0.5
    if tile == 0:
      s_old[:, col] = float("-inf")  # (a spike in tile 0 is measured against the tile's OTHER keys)
    s_old = s_old.max(dim=-1).values
    grown.append(((s_new - s_old) * LOG2E).tolist())
  return q, k, v, grown


def _ref64(q, k, v, scale, visible=None, bias=None):
  """float64 softmax(scale q k^T + bias, masked) v and its natural-log LSE; a row without a visible key: O = NaN, LSE = -inf."""
  s = torch.einsum("bhqd,bhkd->bhqk", q.double(), k.double()) * scale
  if bias is not None:
    s = s + bias.double()
  if visible is not None:
    s = s.masked_fill(~visible, float("-inf"))
  lse = torch.logsumexp(s, dim=-1)
  p = torch.exp(s - lse[..., None])  # (a fully masked row: -inf - -inf = NaN, SDPA's contract)
  return torch.einsum("bhqk,bhkd->bhqd", p, v.double()), lse


def _assert_close(o, lse, o_ref, lse_ref, dtype, name):
  o, o_ref, lse, lse_ref = o.double(), o_ref.double(), lse.double(), lse_ref.double()
  assert torch.equal(torch.isnan(o), torch.isnan(o_ref)), f"{name}: NaN pattern of O"
  fin = ~torch.isnan(o_ref)
  err = (o - o_ref).abs()[fin]
  lim = TOL[dtype] + TOL[dtype] * o_ref.abs()[fin]
  print(f"{name}: max |O - ref| {err.max().item() if err.numel() else 0.0:.3e}")
  assert torch.all(err <= lim), f"{name}: max err {err.max().item():.3e}, worst excess {(err - lim).max().item():.3e}"
  assert torch.equal(torch.isneginf(lse), torch.isneginf(lse_ref)), f"{name}: -inf pattern of LSE"
  lfin = torch.isfinite(lse_ref)
  lerr = (lse - lse_ref).abs()[lfin]
  print(f"{name}: max |LSE - ref| {lerr.max().item() if lerr.numel() else 0.0:.3e}")
  assert torch.all(lerr <= LSE_ATOL + LSE_RTOL * lse_ref.abs()[lfin]), f"{name}: LSE max err {lerr.max().item():.3e}"


def _assert_close_to_oracle(o, lse, q, k, v, dtype, name, **kw):
  qb, dt = fo.torch_to_bits(q)
  kb, _ = fo.torch_to_bits(k)
  vb, _ = fo.torch_to_bits(v)
  _, o32, lse_or = fo.oracle_forward(qb, kb, vb, dt, threshold=THR, **kw)
  _assert_close(o, lse, torch.from_numpy(o32).cuda(), torch.from_numpy(lse_or).cuda(), dtype, name + " (oracle)")


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("D", [128, 256, 320, 512])
def test_a_spike_is_seen_wherever_it_sits(hip, D, dtype, case):
  name, spikes = case
  if hip.tile_config(D)["block_keys"] != BC[D]:
    pytest.skip(f"this build walks D = {D} in tiles of {hip.tile_config(D)['block_keys']} keys, the cases are laid out for {BC[D]}")
  q, k, v, grown = _inputs(D, dtype, spikes)
  for (row, tile, col, gain), g2 in zip(spikes, grown):
    # the case is what it says: far past the threshold, or inside it (in every head)
    assert all(x > 2 * THR for x in g2) if gain is not None else all(0.25 * THR < x < 0.75 * THR for x in g2), (name, g2)
  scale = D ** -0.5
  plan = {}
  o, lse = hip.forward(q, k, v, None, False, scale, plan_out=plan, num_splits=1)
  assert plan["block_keys"] == BC[D] and plan["splits"] == 1 and "m16" in plan["kernel"], plan  # (one workgroup walks all four tiles of a head)
  o_ref, lse_ref = _ref64(q, k, v, scale)
  tag = f"D{D} {dtype} {name}"
  _assert_close(o, lse, o_ref, lse_ref, dtype, tag)
  _assert_close_to_oracle(o, lse, q, k, v, dtype, tag, block_keys=BC[D])
  for row, tile, col, gain in spikes:
    if gain is not None:  # the spiked row is the spiked key's value row, to the weight the other keys keep (e^-20 and less)
      assert torch.allclose(o[0, :, row].float(), v[0, :, tile * BC[D] + col].float(), atol=TOL[dtype], rtol=TOL[dtype]), tag


# ----------------------------------------------------------------------------- the other builds of the tile text, D = 512
D5 = 512


def test_causal_diagonal_tile(hip):
  """is_causal (tail aligned: row r sees keys <= r + 69): a spike in a full tile in front of the diagonal and one ON the ragged diagonal tile."""
  dtype = torch.bfloat16
  q, k, v, _ = _inputs(D5, dtype, [(100, 1, 7, G_FAR), (127, 3, 3, G_FAR)])
  nkv = _nkv(D5)
  o, lse = hip.forward(q, k, v, None, True, D5 ** -0.5, num_splits=1)
  vis = (torch.arange(nkv, device="cuda")[None, :] <= torch.arange(NQ, device="cuda")[:, None] + (nkv - NQ))[None, None]
  o_ref, lse_ref = _ref64(q, k, v, D5 ** -0.5, visible=vis)
  _assert_close(o, lse, o_ref, lse_ref, dtype, "causal")
  _assert_close_to_oracle(o, lse, q, k, v, dtype, "causal", causal=True, block_keys=64)


@pytest.mark.parametrize("hide", ["a_whole_tile", "the_spike"])
def test_boolean_mask(hip, hide):
  """A step whose scores are all -inf (nothing may grow, nothing may turn NaN) in front of the spike's step; and a spike the mask hides (it must not be seen)."""
  dtype = torch.bfloat16
  q, k, v, _ = _inputs(D5, dtype, [(5, 2, 7, G_FAR)])
  nkv = _nkv(D5)
  vis = torch.ones(1, 1, NQ, nkv, dtype=torch.bool, device="cuda")
  if hide == "a_whole_tile":
    vis[..., 64:128] = False
  else:
    vis[0, 0, 5, 2 * 64 + 7] = False
  plan = {}
  o, lse = hip.forward(q, k, v, vis, False, D5 ** -0.5, plan_out=plan, num_splits=1)
  o_ref, lse_ref = _ref64(q, k, v, D5 ** -0.5, visible=vis)
  _assert_close(o, lse, o_ref, lse_ref, dtype, f"mask hides {hide}")
  bias = np.where(vis.cpu().numpy(), 0.0, -np.inf).astype(np.float32)
  _assert_close_to_oracle(o, lse, q, k, v, dtype, f"mask hides {hide}", bias=bias, block_keys=plan["block_keys"])
  if hide == "the_spike":
    assert lse[0, :, 5].max().item() < 10.0  # (the spike alone would make it ~ 30)


def test_key_bias(hip):
  dtype = torch.bfloat16
  q, k, v, _ = _inputs(D5, dtype, [(16, 1, 12, G_FAR)])
  nkv = _nkv(D5)
  g = torch.Generator(device="cuda").manual_seed(5)
  bias = (torch.randn(1, 1, 1, nkv, device="cuda", generator=g) * 0.25).to(dtype)
  plan = {}
  o, lse = hip.forward(q, k, v, bias, False, D5 ** -0.5, plan_out=plan, num_splits=1)
  o_ref, lse_ref = _ref64(q, k, v, D5 ** -0.5, bias=bias)
  _assert_close(o, lse, o_ref, lse_ref, dtype, "key bias")
  _assert_close_to_oracle(o, lse, q, k, v, dtype, "key bias", bias=bias.float().cpu().numpy(), block_keys=plan["block_keys"])


def test_dropout(hip):
  """Dropout 0.1, fixed seed: the LSE is undropped (against float64); O against the oracle, which draws the same Philox keep bits (the bound of
  tests/test_fwd_gpu.py's dropout test)."""
  dtype = torch.bfloat16
  q, k, v, _ = _inputs(D5, dtype, [(31, 1, 15, G_FAR)])
  o, lse = hip.forward(q, k, v, None, False, D5 ** -0.5, dropout_p=0.1, philox_seed=1234567, philox_offset=0, num_splits=1)
  _, lse_ref = _ref64(q, k, v, D5 ** -0.5)
  lerr = (lse.double() - lse_ref).abs()
  assert torch.all(lerr <= LSE_ATOL + LSE_RTOL * lse_ref.abs()), lerr.max().item()
  qb, dt = fo.torch_to_bits(q)
  kb, _ = fo.torch_to_bits(k)
  vb, _ = fo.torch_to_bits(v)
  _, o32, lse_or = fo.oracle_forward(qb, kb, vb, dt, block_keys=64, dropout_p=0.1, philox_seed=1234567, philox_offset=0)
  err = np.abs(o.float().cpu().numpy() - o32)
  print(f"dropout: max err {err.max():.3e} mean {err.mean():.3e}")
  assert err.max() <= 2.0 ** -8 * np.abs(o32).max() + 6e-3 and err.mean() < 6e-4, (err.max(), err.mean())
  np.testing.assert_allclose(lse.float().cpu().numpy(), lse_or, atol=2e-4, rtol=2e-5)


def _packed_pair(dtype):
  """Two sequences (128 rows x 197 keys with a spike, 70 x 133 with another), packed."""
  qa, ka, va, _ = _inputs(D5, dtype, [(15, 2, 0, G_FAR)])
  qb, kb, vb, _ = _inputs(D5, dtype, [(40, 1, 9, G_FAR)], nkv=133, seed=1, nq=70)
  q = torch.cat([qa[0], qb[0]], dim=1).transpose(0, 1).contiguous()  # [T, H, D]
  k = torch.cat([ka[0], kb[0]], dim=1).transpose(0, 1).contiguous()
  v = torch.cat([va[0], vb[0]], dim=1).transpose(0, 1).contiguous()
  cu_q = torch.tensor([0, 128, 198], dtype=torch.int32, device="cuda")
  cu_k = torch.tensor([0, 197, 330], dtype=torch.int32, device="cuda")
  return q, k, v, cu_q, cu_k, ((qa, ka, va), (qb, kb, vb))


def _check_packed(o, lse, seqs, dtype, name):
  r0 = 0
  for i, (qs, ks, vs) in enumerate(seqs):
    n = qs.size(2)
    o_ref, lse_ref = _ref64(qs, ks, vs, D5 ** -0.5)
    _assert_close(o[r0:r0 + n].transpose(0, 1)[None], lse[:, r0:r0 + n][None], o_ref, lse_ref, dtype, f"{name} seq {i}")
    r0 += n


def test_packed_call_with_two_sequences(hip):
  dtype = torch.bfloat16
  q, k, v, cu_q, cu_k, seqs = _packed_pair(dtype)
  o, lse = hip.varlen_forward(q, k, v, cu_q, cu_k, 128, 197, False, D5 ** -0.5, num_splits=1)
  _check_packed(o, lse, seqs, dtype, "packed")


def test_paged_call(hip):
  """The same two sequences, their keys in 64-row pages handed out in reverse order."""
  dtype = torch.bfloat16
  q, k, v, cu_q, cu_k, seqs = _packed_pair(dtype)
  page, ppr, hkv = 64, 4, H
  pk = torch.zeros(2 * ppr, page, hkv, D5, dtype=dtype, device="cuda")
  pv = torch.zeros_like(pk)
  table = torch.arange(2 * ppr - 1, -1, -1, dtype=torch.int32, device="cuda").view(2, ppr).contiguous()
  for i, (lo, hi) in enumerate(((0, 197), (197, 330))):
    for j in range(-(-(hi - lo) // page)):
      rows = slice(lo + j * page, min(lo + (j + 1) * page, hi))
      n = rows.stop - rows.start
      pk[int(table[i, j]), :n] = k[rows]
      pv[int(table[i, j]), :n] = v[rows]
  used = torch.tensor([197, 133], dtype=torch.int32, device="cuda")
  plan = {}
  o, lse = hip.varlen_forward(q, pk, pv, cu_q, None, 128, ppr * page, False, D5 ** -0.5, seqused_k=used, block_table=table, num_splits=1, plan_out=plan)
  assert plan["kernel"].startswith("ffpa_fwd_m16_paged_kernel"), plan
  _check_packed(o, lse, seqs, dtype, "paged")


def test_mla_latent_call(hip):
  """One sequence over the latent pool (keys = the 576-wide rows, values = their first 512 columns): 16 heads x 8 tokens = 128 rows of one latent head, a spike
  in the last full tile for one (token, head)."""
  dtype, D, DV, hq, sq, nkv = torch.bfloat16, 576, 512, 16, 8, 197
  if (D, DV) not in hip.MLA_BUILDS:
    pytest.skip(f"the MLA latent kernel is not built for ({D}, {DV})")
  g = torch.Generator(device="cuda").manual_seed(77)
  q = torch.randn((sq, hq, D), dtype=dtype, device="cuda", generator=g)
  rows = torch.randn((nkv, D), dtype=dtype, device="cuda", generator=g)
  qr = q[3, 9].double()
  rows[2 * 64 + 12] = (G_FAR * math.sqrt(D) * qr / (qr.norm() ** 2)).to(dtype)
  page, ppr = 64, 4
  pool = torch.zeros(ppr, page, 1, D, dtype=dtype, device="cuda")
  table = torch.tensor([[2, 0, 3, 1]], dtype=torch.int32, device="cuda")
  for j in range(ppr):
    n = max(0, min(page, nkv - j * page))
    pool[int(table[0, j]), :n, 0] = rows[j * page:j * page + n]
  cu_q = torch.tensor([0, sq], dtype=torch.int32, device="cuda")
  used = torch.tensor([nkv], dtype=torch.int32, device="cuda")
  o, lse = hip.mla_forward(q, pool, DV, cu_q, used, table, sq, ppr * page, False, D ** -0.5, num_splits=1)
  q4 = q.transpose(0, 1)[None]                       # [1, hq, sq, D]
  k4 = rows[None, None].expand(1, hq, nkv, D)
  o_ref, lse_ref = _ref64(q4, k4, k4[..., :DV], D ** -0.5)
  _assert_close(o.transpose(0, 1)[None], lse[None], o_ref, lse_ref, dtype, "mla")
  assert lse[9, 3].item() > 25.0  # the spike was seen


def test_fully_masked_rows(hip):
  """A row without a visible key: O = NaN in the dense call (SDPA's contract); O = 0 and LSE = -inf in the packed call (its contract) — m_run stays -inf through
  every step, and the exponents subtract 0."""
  dtype = torch.bfloat16
  q, k, v, _ = _inputs(D5, dtype, [(5, 1, 7, G_FAR)])
  nkv = _nkv(D5)
  vis = torch.ones(1, 1, NQ, nkv, dtype=torch.bool, device="cuda")
  vis[0, 0, 5] = False   # the spiked row itself
  vis[0, 0, 77] = False
  o, lse = hip.forward(q, k, v, vis, False, D5 ** -0.5, num_splits=1)
  assert torch.isnan(o[0, :, 5]).all() and torch.isnan(o[0, :, 77]).all()
  o_ref, lse_ref = _ref64(q, k, v, D5 ** -0.5, visible=vis)
  _assert_close(o, lse, o_ref, lse_ref, dtype, "dense, masked rows")
  # packed, causal, 128 rows over 100 keys (tail aligned): rows 0 .. 27 see no key
  qp = q[0].transpose(0, 1).contiguous()
  kp, vp = k[0, :, :100].transpose(0, 1).contiguous(), v[0, :, :100].transpose(0, 1).contiguous()
  cu_q = torch.tensor([0, 128], dtype=torch.int32, device="cuda")
  cu_k = torch.tensor([0, 100], dtype=torch.int32, device="cuda")
  op, lsep = hip.varlen_forward(qp, kp, vp, cu_q, cu_k, 128, 100, True, D5 ** -0.5, num_splits=1)
  assert torch.all(op[:28] == 0) and torch.isneginf(lsep[:, :28]).all()
  visp = (torch.arange(100, device="cuda")[None, :] <= torch.arange(NQ, device="cuda")[:, None] - 28)[None, None]
  o_ref, lse_ref = _ref64(q, k[:, :, :100], v[:, :, :100], D5 ** -0.5, visible=visp)
  _assert_close(op[28:].transpose(0, 1)[None], lsep[:, 28:][None], o_ref[:, :, 28:], lse_ref[:, :, 28:], dtype, "packed, causal")
