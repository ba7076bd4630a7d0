"""A float64 restatement of the KV-cache calls (ffpa_attn_with_kvcache, its append + rotary, ffpa_attn_with_kvcache_cascade), written from the contract in
ffpa_attn_amd/kvcache.py's docstrings and from nothing in the kernels; the allowance every oracle / float64 comparison of the suite uses; builders of the strided
layouts serving engines hand over; and the seeded case generator of the family sweep.  Plain torch (any device) + numpy: importable and testable without a GPU
(tests/test_kvcache_ref.py)."""

from __future__ import annotations

import random

import numpy as np
import torch

TORCH_DTYPE = {"bf16": torch.bfloat16, "fp16": torch.float16}
DTYPE_NAME = {torch.bfloat16: "bf16", torch.float16: "fp16"}
MANT_BITS = {"bf16": 7, "fp16": 10}
PAGED_HEAD_DIM_CLASSES = tuple(range(128, 1025, 64))  # FFPA_FOR_EACH_VARLEN_HEAD_DIM (csrc/ffpa_launch.h): one paged build per class, plain and NT


def _dt(dtype) -> str:
  return dtype if isinstance(dtype, str) else DTYPE_NAME[dtype]


# ----------------------------------------------------------------------------- the allowance
def allowance(ref, pmax, p2sum, v, dtype, noise: bool = True):
  """``(half_ulp, flip)``: what separates a kernel's 16-bit output from an unrounded reference ``ref [..., D]`` (numpy), per element.

  * ``half_ulp``: half a storage ulp of the result (bf16 2^-8, fp16 2^-11, relative; floored at |O| = 2^-6);
  * ``flip``: P entries whose fp32 value sits on a 16-bit rounding boundary and round the other way in the kernel (v_exp_f32 / MFMA summation order vs libm /
    sequential): one flip moves O by ulp x p / l x |v|.  The expression takes the ROW's largest p / l (``pmax [...]``) and the largest |v| — 2.5e-3 at 32 keys
    (p / l ~ 0.1 ... 1: the constant the first tests used everywhere, still the cap), ~ 1e-4 at 8192 keys (p / l ~ 5e-3), where a constant 2.5e-3 would be a
    quarter of an output's standard deviation and could not see a dropped KV tile.  3 x: the kernel's scores differ from the reference's by the fp32 summation
    order of the MFMA — ~ 1e-5 in the log2 domain, about one P entry in 500 on the other side of a boundary: rows of a few hundred keys see a handful of flips
    among their larger entries (1.5 x failed 64 of 1447 cases by up to 3e-4, all at 250 ... 3000 keys).  The cap never cuts below ONE flip of the row's largest
    entry at the largest |v|: a row of two visible keys whose second P entry sits on a rounding midpoint moves by ulp x |v| / l = 7.4e-3 when it rounds the
    other way (packed fuzz seed 1122: p' = 0.55665 between 0.5547 and 0.5586, v = -2.95, oracle -1.3560, kernel -1.3634 -> bf16 -1.3672, exact -1.3596);
  * ``noise``: the 16-bit rounding of P itself, five sigma of both sides, from the row's ``p2sum [...]`` = sum (p / l)^2 and the RMS of v.  It applies wherever the
    reference does not round ITS P entries the way the kernel does: a launch that splits the KV axis (every split rounds against its own running max) against
    the C oracle, and every comparison with a float64 reference, which does not round P at all.

  ``v``: the values the rows read (a tensor / array: its largest |v| and RMS are taken) or the pair ``(vmax, vrms)``."""
  dt = _dt(dtype)
  ulp = 2.0 ** -8 if dt == "bf16" else 2.0 ** -11
  if isinstance(v, tuple):
    vmax, vrms = float(v[0]), float(v[1])
  elif isinstance(v, torch.Tensor):
    vf = v.detach().float()
    vmax, vrms = float(vf.abs().max().item()), float(vf.pow(2).mean().sqrt().item())
  else:
    vf = np.asarray(v, dtype=np.float64)
    vmax, vrms = float(np.abs(vf).max()), float(np.sqrt((vf ** 2).mean()))
  flip_cap = 2.5e-3 if dt == "bf16" else 4e-4
  extra = 0.0
  if noise:
    extra = 5.0 * (0.5 * ulp / np.sqrt(3.0)) * np.sqrt(2.0 * np.nan_to_num(p2sum, nan=1.0)) * vrms
  one_flip = ulp * np.nan_to_num(pmax, nan=1.0) * vmax
  flip = np.minimum(np.maximum(flip_cap, one_flip), np.maximum(3.0 * one_flip, 2e-5) + extra)[..., None] * np.ones_like(ref)
  half_ulp = ulp * np.maximum(np.abs(ref), 2.0 ** -6)
  return half_ulp, flip


LSE_ATOL, LSE_RTOL = 2e-4, 2e-5


def check(out, lse, ref, *, v, dtype, name: str = "", extra=None) -> float:
  """``out [B, Sq, Hq, D]`` (16-bit, any device) and ``lse [B, Hq, Sq] | None`` against ``ref = attend(...)``: every element inside ``allowance`` (with the noise
  term: the reference is float64), 0 exactly where the reference row sees no key, no NaN anywhere, LSE within atol 2e-4 / rtol 2e-5 and -inf in the same
  places.  ``extra`` (numpy, broadcastable to ``out``): a margin the caller has derived for some rows, added to their allowance (tests/model_values.py
  ``absorbed_margin``: rows masked wholly by a large finite value).  Returns the worst error / allowance ratio of the call."""
  o_ref, lse_ref, pmax, p2sum = (t.detach().cpu().numpy() for t in ref)
  got = out.detach().double().cpu().numpy()
  assert got.shape == o_ref.shape, f"{name}: output shape {got.shape}, reference {o_ref.shape}"
  assert np.isfinite(got).all(), f"{name}: {np.count_nonzero(~np.isfinite(got))} non-finite outputs"
  if got.size == 0:
    return 0.0
  stat = lambda t: np.transpose(t, (0, 2, 1))  # [B, Hq, Sq] -> [B, Sq, Hq]: the rows of out
  half_ulp, flip = allowance(o_ref, stat(pmax), stat(p2sum), v, dtype, noise=True)
  err = np.abs(got - o_ref)
  empty = np.isneginf(stat(lse_ref))
  assert (got[empty] == 0).all(), f"{name}: a row without a visible key is not 0"
  bound = half_ulp + flip + (0.0 if extra is None else np.asarray(extra, dtype=np.float64))
  ratio = float((err / bound).max())
  if ratio > 1.0:
    i = np.unravel_index(np.argmax(err / bound), err.shape)
    raise AssertionError(f"{name}: max err {err.max():.3e}; worst error / allowance {ratio:.2f} at [b, token, head, dim] = {tuple(int(x) for x in i)}: got {got[i]:.6f}, "
                         f"float64 {o_ref[i]:.6f}, allowance {bound[i]:.3e}")
  if lse is not None:
    lg = lse.detach().double().cpu().numpy()
    assert lg.shape == lse_ref.shape, f"{name}: LSE shape {lg.shape}, reference {lse_ref.shape}"
    assert np.array_equal(np.isneginf(lg), np.isneginf(lse_ref)), f"{name}: LSE -inf pattern"
    fin = np.isfinite(lse_ref)
    np.testing.assert_allclose(lg[fin], lse_ref[fin], atol=LSE_ATOL, rtol=LSE_RTOL, err_msg=f"{name}: LSE")
  return ratio


# ----------------------------------------------------------------------------- the call, restated
def gather(pool_k, pool_v, table, b: int, n: int):
  """Keys ``[0, n)`` of sequence b -> ``(k [n, Hkv, D], v [n, Hkv, D])``.  Paged (``table [B, pages_per_seq]``): key j is row ``j % page`` of page
  ``clamp(table[b, j // page], 0, num_pages - 1)``; contiguous (``table`` None): row j of slab b.  Indexes the views: any strides."""
  if table is None:
    return pool_k[b, :n], pool_v[b, :n]
  page, num_pages = pool_k.size(1), pool_k.size(0)
  j = torch.arange(n, device=pool_k.device)
  ids = table[b].to(torch.int64)[j // page].clamp(0, num_pages - 1)
  return pool_k[ids, j % page], pool_v[ids, j % page]


def capacity_of(k_cache, table) -> int:
  return k_cache.size(1) if table is None else table.size(1) * k_cache.size(1)


def rotate(x, cos, sin, pos, interleaved: bool):
  """``x [S, H, D]`` rotated in float64: token s at position ``pos[s]`` (clamped to ``seqlen_ro - 1``) of ``cos`` / ``sin [seqlen_ro, rotary_dim / 2]``; the first
  ``rotary_dim`` dims in pairs (2j, 2j + 1) (interleaved) or (j, j + rotary_dim / 2) (GPT-NeoX), the others untouched.  Not rounded."""
  x = x.double()
  half = cos.size(1)
  rd = 2 * half
  p = torch.as_tensor(pos, device=x.device, dtype=torch.int64).clamp(max=cos.size(0) - 1)
  c, s = cos.double()[p][:, None, :], sin.double()[p][:, None, :]  # [S, 1, rd / 2]
  out = x.clone()
  if interleaved:
    x0, x1 = x[..., 0:rd:2], x[..., 1:rd:2]
    out[..., 0:rd:2] = x0 * c - x1 * s
    out[..., 1:rd:2] = x1 * c + x0 * s
  else:
    x0, x1 = x[..., :half], x[..., half:rd]
    out[..., :half] = x0 * c - x1 * s
    out[..., half:rd] = x1 * c + x0 * s
  return out


def append(k_cache, v_cache, k, v, lens, table=None, cos=None, sin=None, interleaved: bool = True, causal: bool = False, q=None):
  """The append of ffpa_attn_with_kvcache, IN PLACE on ``k_cache`` / ``v_cache`` (hand it re-views of a cloned storage: ``reviewed``): key i of sequence b at
  position ``max(len_b, 0) + i``, dropped at or past the capacity; K rotated in float64 and rounded ONCE to the cache's dtype, V copied.
  -> ``(q_rot float64 | None, post-append lengths (list), rotated)``; ``rotated``: ``(b, position)`` of the K rows written through a rotation (the elements a
  kernel that rotates in fp32 may miss by one ulp: their first ``rotary_dim`` dims)."""
  B, snew = k.size(0), k.size(1)
  cap = capacity_of(k_cache, table)
  page = k_cache.size(1)
  lens = [int(x) for x in lens]
  used, rotated = [], []
  for b in range(B):
    base = max(lens[b], 0)
    used.append(min(base + snew, cap))
    pos = [base + i for i in range(snew)]
    kb = rotate(k[b], cos, sin, pos, interleaved).to(k_cache.dtype) if cos is not None and snew else k[b]
    for i, p in enumerate(pos):
      if p >= cap:
        continue
      if table is None:
        slab, row = b, p
      else:
        slab, row = min(max(int(table[b, p // page]), 0), k_cache.size(0) - 1), p % page
      k_cache[slab, row] = kb[i]
      v_cache[slab, row] = v[b, i]
      if cos is not None:
        rotated.append((slab, row))
  q_rot = None
  if cos is not None and q is not None:
    sq = q.size(1)
    q_rot = torch.stack([rotate(q[b], cos, sin, [max(lens[b], 0) + (i if causal else 0) for i in range(sq)], interleaved) for b in range(B)]) if B else q.double()
  return q_rot, used, rotated


def attend(q, k_cache, v_cache, lens, table=None, causal: bool = False, scale: "float | None" = None):
  """Float64 softmax attention of ``q [B, Sq, Hq, D]`` (any float dtype: a float64 rotated q stays unrounded) over the first ``clamp(len_b, 0, capacity)`` keys
  of every sequence: bottom-right causal (query i sees keys j <= i + n - Sq), GQA (query head h reads KV head h // group), rows without a visible key O = 0,
  LSE = -inf.  -> ``(o [B, Sq, Hq, D], lse [B, Hq, Sq], pmax [B, Hq, Sq], p2sum [B, Hq, Sq])`` float64; ``pmax`` the row's largest p / l, ``p2sum`` its
  sum of (p / l)^2 (both 0 for an empty row)."""
  B, sq, hq, d = q.shape
  hkv = k_cache.size(2)
  group = hq // hkv
  cap = capacity_of(k_cache, table)
  scale = d ** -0.5 if scale is None else scale
  dev = q.device
  o = torch.zeros((B, sq, hq, d), dtype=torch.float64, device=dev)
  lse = torch.full((B, hq, sq), float("-inf"), dtype=torch.float64, device=dev)
  pmax = torch.zeros((B, hq, sq), dtype=torch.float64, device=dev)
  p2sum = torch.zeros((B, hq, sq), dtype=torch.float64, device=dev)
  for b in range(B):
    n = min(max(int(lens[b]), 0), cap)
    if n == 0 or sq == 0:
      continue
    kb, vb = gather(k_cache, v_cache, table, b, n)
    kb, vb = kb.double().transpose(0, 1), vb.double().transpose(0, 1)         # [Hkv, n, D]
    qb = q[b].double().transpose(0, 1).reshape(hkv, group * sq, d)             # [Hkv, group x Sq, D], rows (head in group, token)
    s = torch.matmul(qb, kb.transpose(1, 2)) * scale                           # [Hkv, group x Sq, n]
    if causal:
      tok = torch.arange(sq, device=dev).repeat(group)
      hidden = torch.arange(n, device=dev)[None, :] > (tok + (n - sq))[:, None]
      s = s.masked_fill(hidden[None], float("-inf"))
    m = s.amax(dim=-1, keepdim=True)
    live = torch.isfinite(m)
    e = torch.exp(s - torch.where(live, m, torch.zeros_like(m)))
    l = e.sum(dim=-1, keepdim=True)
    p = torch.where(live, e / torch.where(live, l, torch.ones_like(l)), torch.zeros_like(e))
    ob = torch.matmul(p, vb)                                                   # [Hkv, group x Sq, D]
    o[b] = ob.reshape(hq, sq, d).transpose(0, 1)
    row_lse = torch.where(live, m + torch.log(torch.where(live, l, torch.ones_like(l))), torch.full_like(m, float("-inf")))
    lse[b] = row_lse.reshape(hq, sq)
    pmax[b] = p.amax(dim=-1).reshape(hq, sq)
    p2sum[b] = p.pow(2).sum(dim=-1).reshape(hq, sq)
  return o, lse, pmax, p2sum


def visible_values(v_cache, lens, table=None):
  """``(largest |v|, RMS of v)`` over the keys the sequences hold: what ``allowance`` wants of V when the rest of a pool holds NaN."""
  cap = capacity_of(v_cache, table)
  amax, sq, cnt = 0.0, 0.0, 0
  for b in range(len(lens)):
    n = min(max(int(lens[b]), 0), cap)
    if n == 0:
      continue
    vb = gather(v_cache, v_cache, table, b, n)[1].double()
    amax = max(amax, float(vb.abs().max().item()))
    sq += float(vb.pow(2).sum().item())
    cnt += vb.numel()
  return (amax, (sq / cnt) ** 0.5) if cnt else (1.0, 1.0)


def ulp_of(x, dtype):
  """The spacing of ``dtype`` at |x| (float64 tensor): 2^(exponent - mantissa bits), floored at the format's smallest spacing."""
  dt = _dt(dtype)
  _, e = torch.frexp(x.double().abs().clamp_min(1e-300))
  floor = -24 if dt == "fp16" else -133
  return torch.pow(2.0, (e - 1 - MANT_BITS[dt]).clamp_min(floor).double())


def check_cache(got_storage, want_storage, got_view, want_view, rotated, rotary_dim: int, name: str = "") -> None:
  """A cache after an append: the WHOLE owning storage bit-identical to the reference's, but for the first ``rotary_dim`` dims of the rotated K rows
  ``rotated = [(slab or page, row), ...]`` of the view, which may miss the once-rounded float64 rotation by one ulp of the dtype."""
  g, w = got_storage.view(torch.int16), want_storage.view(torch.int16)
  if rotated and rotary_dim:
    idx = torch.tensor(sorted(set(rotated)), dtype=torch.int64, device=got_view.device)
    gr, wr = got_view[idx[:, 0], idx[:, 1]][..., :rotary_dim].double(), want_view[idx[:, 0], idx[:, 1]][..., :rotary_dim].double()
    assert torch.isfinite(gr).all(), f"{name}: a rotated K row is not finite"
    bad = (gr - wr).abs() > ulp_of(wr, got_view.dtype)
    assert not bad.any(), f"{name}: {int(bad.sum())} rotated K elements differ from the float64 rotation by more than one ulp (worst {(gr - wr).abs().max().item():.3e})"
    # ... and everything else — the unrotated dims of those rows, V, every row not appended, whatever else the storage holds — must be the same bits
    mask = torch.zeros_like(want_storage, dtype=torch.bool)
    mview = reviewed(want_view, want_storage, mask)
    mrows = mview[idx[:, 0], idx[:, 1]]
    mrows[..., :rotary_dim] = True
    mview[idx[:, 0], idx[:, 1]] = mrows
    diff = (g != w) & ~mask
  else:
    diff = g != w
  assert not diff.any(), f"{name}: {int(diff.sum())} elements of the cache's storage differ from the reference's (first at flat index {int(diff.flatten().nonzero()[0])})"


# ----------------------------------------------------------------------------- layouts
POOL_LAYOUTS = ("separate", "kv_dim1", "kv_dim0", "head_major", "wide_row", "batch_padded", "v_half_k_dense")
TABLE_LAYOUTS = ("plain", "wide_slice", "transposed")


def reviewed(view, storage, new_storage):
  """The view ``view`` of ``storage`` (a dense tensor that owns its memory) taken of ``new_storage`` (same shape and dtype: a clone, a mask)."""
  off = view.storage_offset() - storage.storage_offset()
  return new_storage.as_strided(view.size(), view.stride(), new_storage.storage_offset() + off)


def lay_out_cache(kc, vc, layout: str, fill: float = float("nan")):
  """The logical caches ``kc`` / ``vc [N, R, Hkv, D]`` (pools: N pages of R rows; contiguous: N slabs of R keys) in one of the layouts serving engines hand over
  -> ``(k_view, v_view, k_storage, v_storage)``; the views hold the logical data, whatever else the storage holds is ``fill``.  One storage holds both when
  K and V are halves of one tensor (``k_storage is v_storage``).

  separate: two dense tensors.  kv_dim1: ``kv[:, 0]`` / ``kv[:, 1]`` of ``[N, 2, R, Hkv, D]`` (page stride doubled; a contiguous cache is not viewable as
  ``[N x R, Hkv, D]``).  kv_dim0: ``kv[0]`` / ``kv[1]`` of ``[2, N, R, Hkv, D]``.  head_major: ``[N, Hkv, R, D]`` viewed as ``[N, R, Hkv, D]``.  wide_row: the
  ``[..., :D]`` slice of rows of D + 24 elements.  batch_padded: the first N of N + 2 slabs / pages.  v_half_k_dense: K a dense tensor, V the ``[:, 1]`` half of
  ``[N, 2, R, Hkv, D]`` — the two page strides differ."""
  N, R, H, D = kc.shape
  new = lambda *shape: torch.full(shape, fill, dtype=kc.dtype, device=kc.device)
  if layout == "separate":
    ks, vs = kc.clone(), vc.clone()
    return ks, vs, ks, vs
  if layout == "v_half_k_dense":
    ks, vs = kc.clone(), new(N, 2, R, H, D)
    vs[:, 1].copy_(vc)
    return ks, vs[:, 1], ks, vs
  if layout == "kv_dim1":
    s = new(N, 2, R, H, D)
    kv_, vv = s[:, 0], s[:, 1]
  elif layout == "kv_dim0":
    s = new(2, N, R, H, D)
    kv_, vv = s[0], s[1]
  elif layout in ("head_major", "wide_row", "batch_padded"):
    shape = {"head_major": (N, H, R, D), "wide_row": (N, R, H, D + 24), "batch_padded": (N + 2, R, H, D)}[layout]
    ks, vs = new(*shape), new(*shape)
    cut = {"head_major": lambda t: t.transpose(1, 2), "wide_row": lambda t: t[..., :D], "batch_padded": lambda t: t[:N]}[layout]
    kv_, vv = cut(ks), cut(vs)
    kv_.copy_(kc)
    vv.copy_(vc)
    return kv_, vv, ks, vs
  else:
    raise ValueError(layout)
  kv_.copy_(kc)
  vv.copy_(vc)
  return kv_, vv, s, s


def lay_out_qkv(q, k, v, fused: bool):
  """``q [B, S, Hq, D]`` and the new ``k`` / ``v [B, S, Hkv, D]`` as slices of one fused QKV projection ``[B, S, Hq + 2 Hkv, D]`` (same S), or as they are."""
  if fused and k is None:
    return torch.cat((q, torch.zeros_like(q[:, :, :2])), dim=2)[:, :, :q.size(2)], k, v
  if not fused or q.size(1) != k.size(1):
    return q, k, v
  hq, hkv = q.size(2), k.size(2)
  s = torch.cat((q, k, v), dim=2)
  return s[:, :, :hq], s[:, :, hq:hq + hkv], s[:, :, hq + hkv:]


def lay_out_table(table, layout: str):
  """An int32 block table as it is, as ``wide[:, 3:3 + n]`` of a wider table (the other columns hold ids far outside any pool), or with a non-unit column stride."""
  if layout == "plain":
    return table.contiguous()
  if layout == "wide_slice":
    wide = torch.full((table.size(0), table.size(1) + 7), 2 ** 30, dtype=torch.int32, device=table.device)
    wide[:, 3:3 + table.size(1)] = table
    return wide[:, 3:3 + table.size(1)]
  if layout == "transposed":
    return table.t().contiguous().t()
  raise ValueError(layout)


def lay_out_lens(lens, strided: bool):
  """int32 lengths as they are, or as ``buf[::2]`` (the gaps hold a length that would run far past any cache)."""
  if not strided:
    return lens.contiguous()
  buf = torch.full((2 * lens.numel(),), 2 ** 30, dtype=torch.int32, device=lens.device)
  buf[::2] = lens
  return buf[::2]


# ----------------------------------------------------------------------------- the sweep's cases
ENTRIES = ("plain", "append", "append_rotary", "cascade")
PAGES = (64, 128, 256, 0)  # 0: a contiguous cache
HEADS = ((8, 8), (32, 8), (16, 1), (8, 4), (1, 1))
SPLITS = (0, 1, 2, 5)
STREAMS = ("auto", "on", "off")
SWEEP_SEEDS = tuple(range(60))


def _cycle(seed: int, n: int, mult: int = 1, shift: int = 0) -> int:
  """Axis values are CYCLED over the seeds (co-prime strides per axis), not drawn: every value of every axis appears, whatever the seed list's length >= a few
  periods; what varies freely (lengths, in-between head dims, data) is drawn from the seed's own generator."""
  return (seed * mult + seed // n + shift) % n


def draw_case(seed: int) -> dict:
  """The sweep's case of a seed: plain Python values only (no tensor, no device)."""
  rng = random.Random(seed * 7919 + 13)
  c = {"seed": seed}
  cls = PAGED_HEAD_DIM_CLASSES[seed % 15]
  c["dtype"] = ("bf16", "fp16")[(seed // 15) % 2]
  c["page"] = page = PAGES[(seed // 30 + seed % 15 + (seed // 15) % 2) % 4]
  # a built class itself, or an in-between multiple of 8 that runs on it (8 ... 120 run on the 128 build)
  c["D"] = D = cls if rng.random() < 0.6 else rng.randrange(cls - 56 if cls > 128 else 8, cls, 8)
  c["head_dim_class"] = cls
  c["entry"] = entry = ENTRIES[_cycle(seed, 4)]
  c["layout"] = POOL_LAYOUTS[_cycle(seed, 7, 5, 1)]
  c["table_layout"] = TABLE_LAYOUTS[_cycle(seed, 3, 2, 1)] if page else "plain"
  c["lens_strided"] = bool(_cycle(seed, 2, 1, 1))
  c["fused_qkv"] = bool(_cycle(seed // 2, 2))
  c["heads"] = hq, hkv = HEADS[_cycle(seed, 5, 3)]
  c["B"] = B = 1 + _cycle(seed, 9, 4, 2)
  c["num_splits"] = SPLITS[_cycle(seed, 4, 3, 1)]
  c["stream"] = STREAMS[_cycle(seed, 3)]
  c["causal"] = bool(_cycle(seed, 2))
  c["return_lse"] = rng.random() < 0.75  # (the reference's LSE is compared whenever it is returned)
  chunk = seed % 10 == 7  # occasionally a prefill chunk instead of a few tokens
  c["Sq"] = sq = rng.randrange(65, 301) if chunk else 1 + _cycle(seed, 6, 5, 3)
  append_ = entry in ("append", "append_rotary") or (entry == "cascade" and seed % 8 >= 4)
  c["Snew"] = snew = (sq if (c["fused_qkv"] or rng.random() < 0.5) else rng.choice((0, 1, 3, 70))) if append_ else None
  rotary = entry == "append_rotary" or (entry == "cascade" and seed % 8 >= 6)
  rds = [r for r in (16, D // 2 // 16 * 16, D // 16 * 16) if 0 < r <= D]
  c["rotary_dim"] = rd = rng.choice(rds) if rotary and rds else 0  # (0: a head dim too small to rotate: the entry appends without rotary)
  c["interleaved"] = rng.random() < 0.5
  # the capacity: pages_per_seq pages, or a contiguous slab
  unit = page if page else 64
  long_ = rng.random() < 0.2
  reach = rng.randrange(2500, 6000) if long_ else rng.randrange(100, 1400)
  if chunk:
    reach = max(reach, sq + 64)
  if entry == "cascade":
    reach = max(reach, 2 * (sq + (snew or 0)) + 2 * unit)  # (room for a prefix of up to half the capacity, the step's tokens behind it)
  pps = -(-reach // unit) + 1
  c["pages_per_seq"] = pps
  c["capacity"] = cap = pps * unit if page else reach + rng.randrange(0, 64)
  c["seqlen_ro"] = cap if rng.random() < 0.5 else cap + rng.randrange(1, 100)
  c["shared_prefix_len"] = P = 0
  if entry == "cascade":
    P = unit * rng.randrange(1, max(2, (cap // 2) // unit)) if page else rng.randrange(1, cap // 2)
    c["shared_prefix_len"] = P
    c["cascade"] = True
    room = cap - P - sq - (snew or 0)
    c["lens"] = [P + sq + rng.randrange(0, max(1, room)) for _ in range(B)]
  else:
    edges = (0, -3, 1, unit - 1, unit, unit + 1, cap, cap + 5, cap - 1)
    c["lens"] = [rng.choice(edges) if rng.random() < 0.3 else rng.randrange(1, cap) for _ in range(B)]
    if sum(1 for n in c["lens"] if n > 0) == 0 and rng.random() < 0.8:
      c["lens"][0] = rng.randrange(1, cap)
  # page ids outside the pool: in the entries past a sequence's last used page (never read), and — plain calls only — in a used entry (the documented clamp)
  c["bad_unused_ids"] = bool(page) and rng.random() < 0.5
  c["bad_used_id"] = bool(page) and entry == "plain" and rng.random() < 0.2
  c["share_prefix_pages"] = bool(page) and entry == "plain" and B >= 2 and rng.random() < 0.4
  return c


def effective_lens(c: dict) -> list:
  """Keys every sequence attends over: clamp(len, 0, capacity), after the append where there is one."""
  cap = c["capacity"]
  if c["Snew"] is None:
    return [min(max(n, 0), cap) for n in c["lens"]]
  return [min(max(n, 0) + c["Snew"], cap) for n in c["lens"]]


def visible_rows(c: dict) -> tuple:
  """``(query rows that see at least one key, query rows)`` per query head of a case."""
  seen = 0
  for n in effective_lens(c):
    seen += min(c["Sq"], n) if c["causal"] else (c["Sq"] if n > 0 else 0)
  return seen, c["B"] * c["Sq"]


def materialize(c: dict, device="cpu") -> dict:
  """The tensors of a drawn case on ``device``, in its layouts: ``q, k_cache, v_cache, k_storage, v_storage, k, v, cos, sin, lens, table`` (+ the call's keyword
  arguments under ``kwargs``).  The pool's unused pages — and everything of a storage outside its views — hold NaN."""
  g = torch.Generator().manual_seed(c["seed"] + 1000)
  dev = torch.device(device)
  gd = torch.Generator(device=dev).manual_seed(c["seed"] + 1000)  # (the data is drawn on the device that holds it: a serving-size pool is gigabytes)
  dtype = TORCH_DTYPE[c["dtype"]]
  D, (hq, hkv), B, sq, page, cap = c["D"], c["heads"], c["B"], c["Sq"], c["page"], c["capacity"]
  rnd = lambda *shape: torch.randn(shape, generator=gd, device=dev, dtype=torch.float32 if dev.type == "cpu" else dtype).to(dtype)
  q = rnd(B, sq, hq, D)
  k = v = None
  if c["Snew"] is not None:
    k, v = rnd(B, c["Snew"], hkv, D), rnd(B, c["Snew"], hkv, D)
  table = None
  P = c["shared_prefix_len"]
  if page:
    pps = c["pages_per_seq"]
    shared = P // page
    n_pages = B * (pps - shared) + shared + 3
    ids = torch.randperm(n_pages, generator=g).tolist()
    table = torch.empty((B, pps), dtype=torch.int32)
    nxt = shared
    for b in range(B):
      for j in range(pps):
        if j < shared:
          table[b, j] = ids[j]
        else:
          table[b, j] = ids[nxt]
          nxt += 1
    kc, vc = rnd(n_pages, page, hkv, D), rnd(n_pages, page, hkv, D)
    eff = effective_lens(c)
    if c["share_prefix_pages"]:
      for j in range(min(eff[0], eff[1]) // page):  # sequence 1 reads its first whole pages from sequence 0's ids
        table[1, j] = table[0, j]
    if c["bad_used_id"]:
      b = max(range(B), key=lambda i: eff[i])
      if eff[b] > 0:  # clamps to the pool's first / last page: give it data
        table[b, 0] = -7 if c["seed"] % 2 else n_pages + 11
    for b in range(B):
      first_unused = -(-max(eff[b], min(max(c["lens"][b], 0), cap)) // page)
      for j in range(first_unused, pps):
        if c["bad_unused_ids"]:
          table[b, j] = (-1, n_pages, 2 ** 31 - 1, -(2 ** 31))[(b + j) % 4]
    used_pages = set()
    for b in range(B):
      for j in range(-(-eff[b] // page)):
        used_pages.add(min(max(int(table[b, j]), 0), n_pages - 1))
    unused = torch.ones(n_pages, dtype=torch.bool)
    unused[sorted(used_pages)] = False
    kc[unused.to(dev)] = float("nan")
    vc[unused.to(dev)] = float("nan")
  else:
    kc, vc = rnd(B, cap, hkv, D), rnd(B, cap, hkv, D)
    if P:
      kc[:, :P] = kc[0, :P]
      vc[:, :P] = vc[0, :P]
  cos = sin = None
  if c["rotary_dim"]:
    ang = torch.rand((c["seqlen_ro"], c["rotary_dim"] // 2), generator=g, dtype=torch.float64) * 6.283185307179586
    cos, sin = torch.cos(ang).to(dtype), torch.sin(ang).to(dtype)
  lens = torch.tensor(c["lens"], dtype=torch.int32)
  to = lambda t: None if t is None else t.to(dev)
  q, k, v, kc, vc, cos, sin, lens, table = (to(t) for t in (q, k, v, kc, vc, cos, sin, lens, table))
  kview, vview, ks, vs = lay_out_cache(kc, vc, c["layout"])
  q, k, v = lay_out_qkv(q, k, v, c["fused_qkv"])
  if table is not None:
    table = lay_out_table(table, c["table_layout"])
  lens = lay_out_lens(lens, c["lens_strided"])
  return {"q": q, "k_cache": kview, "v_cache": vview, "k_storage": ks, "v_storage": vs, "k": k, "v": v, "cos": cos, "sin": sin, "lens": lens, "table": table}


def reference(c: dict, t: dict):
  """The float64 result of a case on clones of its storages -> ``(attend's tuple, k_view, v_view, k_storage, v_storage after the append, rotated rows)``."""
  ks = t["k_storage"].clone()
  vs = ks if t["v_storage"] is t["k_storage"] else t["v_storage"].clone()
  kview, vview = reviewed(t["k_cache"], t["k_storage"], ks), reviewed(t["v_cache"], t["v_storage"], vs)
  q, lens, rotated = t["q"], c["lens"], []
  if t["k"] is not None:
    q_rot, lens, rotated = append(kview, vview, t["k"], t["v"], c["lens"], t["table"], t["cos"], t["sin"], c["interleaved"], c["causal"], q=t["q"])
    if q_rot is not None:
      q = q_rot.to(t["q"].dtype)  # (the rotated copy that attends has q's dtype: rounded once)
  return attend(q, kview, vview, lens, t["table"], c["causal"]), kview, vview, ks, vs, rotated
