"""``ffpa_attn_fp8_func`` / ``ffpa_attn_fp8_codes`` on the GPU: the pre-pass byte for byte against ``quantize_attn_fp8``; the attention kernel EXACTLY on
integer codes and power-of-two scales; the public call on model values against float64 attention over the helper's dequantised operands, inside the allowance
DESIGN derives, and end to end against float64 attention on the original inputs, next to the bf16 kernel; torch.compile and a HIP-graph replay."""

import numpy as np
import pytest
import torch

import model_values as mv
from ffpa_attn_amd import ffpa_attn_fp8_codes, ffpa_attn_fp8_func, pack_attn_fp8_k, pack_attn_fp8_q, pack_attn_fp8_vt, quantize_attn_fp8
from ffpa_attn_amd.interface import FP8_BLOCK_KEYS as K, FP8_BLOCK_ROWS as R, FP8_P_SHIFT
from fwd_fp8_cases import attend2, check_against_dequantised, fp8_allowance  # noqa: F401  (moved there unchanged; the edge tests share them)
from test_fwd_gpu import hip  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu
E4M3 = torch.float8_e4m3fn
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}


# ----------------------------------------------------------------------------- 1. the pre-pass writes the helper's bytes
@pytest.mark.parametrize("smooth_k", [True, False])
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("D", [256, 320, 512])
def test_prepass_is_the_helper(hip, D, dtype, smooth_k):
  shape = (2, 4, 1, R + 5, 2 * K + 37, D)
  q, k, v = mv.outliers(shape, DTYPES[dtype], seed=D)
  scale = 1.3 * D ** -0.5
  want = quantize_attn_fp8(q, k, v, scale, smooth_k)
  got = hip.fp8_quantize(q.cuda(), k.cuda(), v.cuda(), scale * mv.LOG2E, smooth_k)
  for name, g, w in zip(want._fields, got, want[:6]):
    assert g.shape == w.shape and g.dtype == w.dtype, name
    diff = g.cpu() != w
    assert not bool(diff.any()), f"{name}: {int(diff.sum())} of {diff.numel()} differ, first at {diff.flatten().nonzero()[0].item()}"


# ----------------------------------------------------------------------------- 2. exact arithmetic through the codes-level entry
# ("Nq > Nkv": under causal the first Nq - Nkv >= one row tile of rows see nothing — the first workgroup walks no key tile at all)
EXACT_SHAPES = {"tile+tail": (R + 5, 2 * K + 3), "one row": (1, 3 * K), "Nq > Nkv": (2 * R + 3, R - 3)}


@pytest.mark.parametrize("group", [1, 4])
@pytest.mark.parametrize("shape", list(EXACT_SHAPES))
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("D", [256, 320, 512])
def test_exact_on_integer_codes(hip, D, causal, shape, group):
  nq, nkv = EXACT_SHAPES[shape]
  B, hkv = 2, 2
  hq = hkv * group
  g = torch.Generator().manual_seed(D + nq + group)
  # q: two columns of 1 per row, a chunk apart; k: codes in {-1, 0} and +1 on the row's own column at ONE key, the row's carrier: it lifts that key's score
  # above the row's other keys' (score collisions aside), and the carriers of all (batch, head, row) together are EVERY key where there are enough rows
  # (asserted): every lane position of the permutation, every key tile.  v: integers in [-4, 4].  Raw scores lie in [-2, 2], q_scale k_scale in {1, 2}: a
  # spread of at most 8
  rows = torch.arange(nq)
  col = (rows[None, None] * 37 + torch.arange(hq)[None, :, None] * 11 + torch.arange(B)[:, None, None] * 5) % D
  qc = torch.zeros(B, hq, nq, D)
  qc.scatter_(-1, col[..., None], 1.0)
  qc.scatter_(-1, ((col + 131) % D)[..., None], 1.0)
  kc = -torch.randint(0, 2, (B, hkv, nkv, D), generator=g).float()
  carrier = ((rows[None, None] + nq * (torch.arange(B)[:, None, None] * hq + torch.arange(hq)[None, :, None])) * 29 + 5) % nkv  # [B, hq, nq]; 29 is coprime to every nkv here
  for b in range(B):
    for h in range(hq):
      kc[b, h // group, carrier[b, h], col[b, h]] = 1.0
  vc = torch.randint(-4, 5, (B, hkv, nkv, D), generator=g).float()
  tiles = lambda n, blk: -(-n // blk)
  q_scale = torch.full((B, hq, tiles(nq, R)), 2.0)
  k_scale = 2.0 ** -torch.randint(0, 2, (B, hkv, tiles(nkv, K)), generator=g).float()
  v_scale = 2.0 ** torch.randint(-1, 2, (B, hkv, D), generator=g).float()
  qh = qc * q_scale.repeat_interleave(R, -1)[..., :nq, None]
  kh = kc * k_scale.repeat_interleave(K, -1)[..., :nkv, None]
  want, p, live, s = attend2(qh, kh, vc * v_scale[:, :, None, :], causal)
  # the conditions under which every step of the kernel is exact in fp32, asserted on the inputs: integer scores; a spread so small that p 2^shift is an integer
  # (so a normal e4m3 with at most 4 significant bits ... a power of two) and the sums of p 2^shift |v| and of p stay below 2^24 units
  fin = torch.isfinite(s)
  assert bool((s[fin] == s[fin].round()).all())
  spread = (torch.where(fin, s, s.new_full((), float("inf"))).amin(-1) - s.amax(-1))[live[..., 0]].abs().max()
  assert spread <= FP8_P_SHIFT and nkv * 4 * 2 ** FP8_P_SHIFT < 2 ** 24
  assert int(carrier.unique().numel()) == min(B * hq * nq, nkv) and (shape == "one row" or B * hq * nq >= nkv)
  out = ffpa_attn_fp8_codes(pack_attn_fp8_q(qc.to(E4M3)).cuda(), q_scale.cuda(), pack_attn_fp8_k(kc.to(E4M3)).cuda(), k_scale.cuda(),
                            pack_attn_fp8_vt(vc.to(E4M3)).cuda(), v_scale.cuda(), seqlen_q=nq, seqlen_kv=nkv, is_causal=causal, out_dtype=torch.bfloat16)
  # (the kernel's one division is IEEE in fp32: the float64 quotient rounded to fp32, then to the output)
  bad = out.cpu() != want.float().to(torch.bfloat16)
  assert not bool(bad.any()), f"{int(bad.sum())} of {bad.numel()} elements differ, worst by {float((out.cpu().double() - want)[bad].abs().max()):.3e}, first at {bad.nonzero()[0].tolist()}"
  if causal and nq > nkv:
    assert not bool(live[:, :, : nq - nkv].any()) and bool((out[:, :, : nq - nkv] == 0).all())


# ----------------------------------------------------------------------------- 3. model values, the derived allowance
FAMILIES = ("outliers", "sink", "peaked", "large_logits", "staircase_up", "staircase_down")


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("D,dtype", [(320, "bf16"), (512, "fp16")])
def test_model_values(hip, D, dtype, family, causal):
  knobs = {"block_keys": K} if family.startswith("staircase") else {}
  q, k, v = mv.FAMILIES[family]((1, 4, 1, 129, 513, D), DTYPES[dtype], 1000 + D, **knobs)
  out = ffpa_attn_fp8_func(q.cuda(), k.cuda(), v.cuda(), is_causal=causal, enable_gqa=True)
  assert out.dtype == q.dtype and out.shape == q.shape
  ratio, _, _ = check_against_dequantised(out, q, k, v, None, causal, True, f"{family} D{D} {dtype} causal={causal}")
  assert ratio <= 1.0


# ----------------------------------------------------------------------------- 4. torch.compile, a HIP graph
def test_compiles_fullgraph(hip):
  q, k, v = (t.cuda() for t in mv.plain((1, 2, 2, 70, 200, 256), torch.bfloat16, 3))
  f = torch.compile(lambda a, b, c: ffpa_attn_fp8_func(a, b, c, is_causal=True), fullgraph=True)
  assert torch.equal(f(q, k, v), ffpa_attn_fp8_func(q, k, v, is_causal=True))


def test_graph_replay_follows_inputs(hip):
  shape = (1, 4, 2, 70, 200, 384)
  q, k, v = (t.cuda() for t in mv.plain(shape, torch.float16, 5))
  call = lambda: ffpa_attn_fp8_func(q, k, v, enable_gqa=True, smooth_k=True)
  side = torch.cuda.Stream()
  with torch.cuda.stream(side):
    call()
  torch.cuda.current_stream().wait_stream(side)
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    out = call()
  for seed in (7, 8, 9):
    for dst, src in zip((q, k, v), mv.peaked(shape, torch.float16, seed)):
      dst.copy_(src)
    graph.replay()
    assert torch.equal(out, call())


# ----------------------------------------------------------------------------- 5. end to end: the original 16-bit inputs, next to the bf16 kernel
@pytest.mark.parametrize("smooth_k", [True, False])
@pytest.mark.parametrize("family", ("plain",) + FAMILIES)
def test_end_to_end_error(hip, family, smooth_k):
  """Against float64 attention on the ORIGINAL inputs the call owes, by the triangle inequality, the quantiser's own error — float64 attention on the
  dequantised operands against float64 attention on the originals, which no kernel can undo — plus the allowance of ``test_model_values``; that and nothing
  else is asserted, element by element.  The figures, next to the bf16 kernel's on the same tensors, are printed (profiles/r38_fwd_fp8.md records them)."""
  D, dtype = 512, torch.bfloat16
  knobs = {"block_keys": K} if family.startswith("staircase") else {}
  q, k, v = mv.FAMILIES[family]((1, 4, 1, 129, 513, D), dtype, 2000 + D, **knobs)
  qc, kc, vc = q.cuda(), k.cuda(), v.cuda()
  out = ffpa_attn_fp8_func(qc, kc, vc, enable_gqa=True, smooth_k=smooth_k)
  name = f"{family} smooth_k={smooth_k}"
  ratio, bound, want = check_against_dequantised(out, q, k, v, None, False, smooth_k, name)
  ref = mv.attend(q, k, v)[0].transpose(1, 2).numpy()
  bf16 = hip.forward(qc, kc, vc, None, False, D ** -0.5, return_lse=False)[0]
  err = lambda x: np.abs(x - ref)
  e_fp8, e_quant, e_bf16 = err(out.double().cpu().numpy()), err(want.numpy()), err(bf16.double().cpu().numpy())
  rms = float(np.sqrt((ref ** 2).mean()))
  print(f"{name}: rms |O| {rms:.3e}; max / rms error  fp8 call {e_fp8.max():.3e} / {np.sqrt((e_fp8 ** 2).mean()):.3e}  quantiser alone {e_quant.max():.3e} / "
        f"{np.sqrt((e_quant ** 2).mean()):.3e}  bf16 kernel {e_bf16.max():.3e} / {np.sqrt((e_bf16 ** 2).mean()):.3e}")
  assert bool((e_fp8 <= e_quant + bound).all()), f"{name}: {int((e_fp8 > e_quant + bound).sum())} elements past quantiser error + allowance"
