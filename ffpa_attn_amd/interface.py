"""Public entry point: ``ffpa_attn_func`` with the ``scaled_dot_product_attention`` signature.

Drop-in for the reference's ``ffpa_attn_func`` (``src/ffpa_attn/ffpa_attn_interface.py:71-189``):
same positional/keyword arguments, same SDPA short-circuit for what the fused kernel does not
serve (small D, D > 1024, short sequences; ``functional.py:676-724``), same validation errors,
and — for everything else — the hand-written gfx950 kernel behind ``ffpa_attn::_fwd_hip``.
"""

from __future__ import annotations

from typing import NamedTuple

import torch

from . import hip  # noqa: F401  (registers the ffpa_attn:: ops the FP8 calls go through)
from .hip import FP8_BLOCK_KEYS, FP8_BLOCK_ROWS, FP8_HEAD_DIMS, FP8_P_SHIFT  # the FP8 forward's tiles, P factor and head dims: stated once, there
from .functional import FFPAAttnMeta


def _reserve_dropout_rng(query: torch.Tensor, key: torch.Tensor, dropout_p: float) -> tuple[int, int]:
  """(seed, offset) for this call's dropout, advancing the device generator by one Philox output per logical
  score, rounded up to a multiple of four — what SDPA's efficient attention reserves and what the reference
  does (functional.py:518-540)."""
  if dropout_p <= 0.0:
    return 0, 0
  with torch.cuda.device(query.device):
    seed = int(torch.cuda.initial_seed())
    offset = int(torch.cuda._get_rng_state_offset())
    elems = query.size(0) * query.size(1) * query.size(2) * key.size(2)
    torch.cuda._set_rng_state_offset(offset + (elems + 3) // 4 * 4)
  return seed, offset


class _FFPAAttnFunc(torch.autograd.Function):
  """HIP forward + SDPA-style backward (the reference's ``_FFPAAttnFunc`` with ``forward_backend`` =
  native kernel and ``backward_backend="sdpa"``, functional.py:964-1172).  O and the natural-log LSE
  ``[B, Hq, Nq]`` are saved only when a gradient is needed (functional.py:1066-1077)."""

  @staticmethod
  def forward(ctx, query, key, value, attn_bias, meta: FFPAAttnMeta):
    from .hip import ffpa_attn_forward_hip

    thr = getattr(meta.forward_meta, "rescale_threshold", None)
    seed, offset = _reserve_dropout_rng(query, key, meta.attn_meta.dropout_p)
    out, lse = ffpa_attn_forward_hip(
      query,
      key,
      value,
      attn_bias,
      causal=meta.attn_meta.is_causal,
      softmax_scale=meta.attn_meta.scale,
      dropout_p=meta.attn_meta.dropout_p,
      philox_seed=seed,
      philox_offset=offset,
      rescale_threshold=-1.0 if thr is None else float(thr),
      kv_bounds=getattr(meta.forward_meta, "kv_bounds", None) if attn_bias is not None else None,
    )
    needs_grad = meta.attn_meta.is_grad_enabled and any(
      t is not None and t.requires_grad for t in (query, key, value, attn_bias)
    )
    if needs_grad:
      ctx.save_for_backward(query, key, value, out, lse, attn_bias)
      ctx.causal = meta.attn_meta.is_causal
      ctx.scale = meta.attn_meta.scale
      ctx.dropout = (meta.attn_meta.dropout_p, seed, offset) if meta.attn_meta.dropout_p > 0.0 else None
      ctx.backward_backend = meta.backward_meta.name
    return out

  @staticmethod
  def backward(ctx, grad_out):
    from .backward import attention_backward, hip_backward_refusal

    query, key, value, out, lse, attn_bias = ctx.saved_tensors
    want_bias = attn_bias is not None and ctx.needs_input_grad[3]
    # backward_backend="hip": the backward kernel where it serves the call (head dims 513 ... 1024, no mask / dropout), today's route everywhere else
    force = "hip" if ctx.backward_backend == "hip" and hip_backward_refusal(query, key, attn_bias=attn_bias, dropout=ctx.dropout) is None else None
    dq, dk, dv, dbias = attention_backward(
      grad_out.contiguous(), query, key, value, out, lse, causal=ctx.causal, scale=ctx.scale, attn_bias=attn_bias,
      want_bias_grad=want_bias, dropout=ctx.dropout, force=force,
    )
    return dq, dk, dv, dbias, None


def _plain_call(query, key, value, attn_bias) -> bool:
  """May this call skip the dispatcher?  Only when nobody is listening on it and every tensor is a plain ``torch.Tensor``: fake / functional /
  subclass tensors (the mask included — it reaches ctypes as a raw pointer), an active ``TorchDispatchMode`` (FlopCounterMode, profiler op records,
  FakeTensorMode) and functorch transforms (vmap's BatchedTensor has type ``torch.Tensor``) all go through the registered op
  ``ffpa_attn::_fwd_hip``, which has the rules for them."""
  if not (type(query) is torch.Tensor and type(key) is torch.Tensor and type(value) is torch.Tensor):
    return False
  if attn_bias is not None and type(attn_bias) is not torch.Tensor:
    return False
  if torch._C._len_torch_dispatch_stack() != 0:
    return False
  if torch._C._functorch.peek_interpreter_stack() is not None:
    return False
  return True


@torch._dynamo.disable
def _ffpa_apply(query, key, value, attn_bias, meta: FFPAAttnMeta) -> torch.Tensor:
  """Graph-break boundary, as the reference's ``_ffpa_apply`` (functional.py:1195-1216).  A call nothing will ever differentiate —
  inference: grad mode off, or no input requires a gradient — goes straight to the launch wrapper: no autograd node, no dispatcher
  round trip, no LSE tensor (what a decode step that synchronises per token pays on the host)."""
  needs_grad = meta.attn_meta.is_grad_enabled and any(t is not None and t.requires_grad for t in (query, key, value, attn_bias))
  if not needs_grad and query.is_cuda and _plain_call(query, key, value, attn_bias):
    from . import hip

    thr = getattr(meta.forward_meta, "rescale_threshold", None)
    seed, offset = _reserve_dropout_rng(query, key, meta.attn_meta.dropout_p)
    return hip.forward(query, key, value, attn_bias, meta.attn_meta.is_causal, meta.attn_meta.scale, dropout_p=meta.attn_meta.dropout_p,
                       philox_seed=seed, philox_offset=offset, rescale_threshold=-1.0 if thr is None else float(thr), return_lse=False,
                       kv_bounds=getattr(meta.forward_meta, "kv_bounds", None) if attn_bias is not None else None)[0]
  return _FFPAAttnFunc.apply(query, key, value, attn_bias, meta)


def ffpa_attn_func(
  query: torch.Tensor,
  key: torch.Tensor,
  value: torch.Tensor,
  attn_mask: torch.Tensor | None = None,
  dropout_p: float = 0.0,
  is_causal: bool = False,
  scale: float | None = None,
  enable_gqa: bool = False,
  **kwargs: object,
) -> torch.Tensor:
  """Fused attention forward for large head dims (``256 < D <= 1024``) on MI355X.

  ``query`` is ``[B, Hq, Nq, D]``; ``key`` / ``value`` are ``[B, Hkv, Nkv, D]`` (``Hq % Hkv == 0``,
  pass ``enable_gqa=True`` when they differ); fp16 or bf16.  ``attn_mask`` follows SDPA
  (bool = keep, float = additive, broadcastable to ``[B, Hq, Nq, Nkv]``) and excludes
  ``is_causal``.  Finite mask values, ``finfo(dtype).min`` included, behave as in SDPA:
  only ``-inf`` or ``False`` hides a key.  ``is_causal=True`` masks ``key > row + (Nkv - Nq)`` (queries aligned to the KV
  tail — FlashAttention's convention, NOT SDPA's top-left one) and requires ``Nkv >= Nq``.
  ``scale`` defaults to ``1/sqrt(D)``.

  Masks: the kernel clips its KV walk to the key ranges of ``attn_mask`` and skips the mask reads where the mask is neutral (an explicit causal
  mask then costs what ``is_causal`` costs).  The ranges come from a scan kernel — a full read of the mask — that runs on EVERY call with a mask
  worth scanning; a serving loop with a static mask should scan once (``hip.mask_kv_bounds(mask, Nq, Nkv)``) and pass the result as
  ``forward_backend=HIPBackend(forward=True, kv_bounds=ranges)`` (or ``TritonBackend`` / ``CUDABackend``: the field exists on all three), or opt
  into the per-tensor cache with ``FFPA_HIP_MASK_BOUNDS_CACHE=1`` (safe only for masks written through torch ops alone: ``hip.forward``).

  Extra keywords: ``backend``, ``forward_backend``, ``backward_backend`` — a name
  (``"hip"``, ``"cuda"``, ``"triton"``, ``"cutedsl"``, ``"sdpa"``) or a
  :class:`~ffpa_attn_amd.backends.Backend` instance.  Anything else raises ``TypeError``.

  Calls the kernel does not serve go to ``torch._C._nn.scaled_dot_product_attention`` directly
  (never through ``F.scaled_dot_product_attention``, so monkey-patching that symbol with this
  function cannot recurse — tests/test_monkey_patch.py:65-69 in the reference).
  """
  meta = FFPAAttnMeta.from_kwargs(**kwargs)
  if meta.fallback(query, key, attn_mask, dropout_p, is_causal=is_causal):
    return torch._C._nn.scaled_dot_product_attention(
      query,
      key,
      value,
      attn_mask=attn_mask,
      dropout_p=dropout_p,
      is_causal=is_causal,
      scale=scale,
      enable_gqa=enable_gqa,
    )
  meta, query, key, value, attn_bias = meta.normalize(
    query, key, value, attn_mask, dropout_p, is_causal, scale, enable_gqa
  )
  return _ffpa_apply(query, key, value, attn_bias, meta)


def ffpa_attn_varlen_func(
  q: torch.Tensor,
  k: torch.Tensor,
  v: torch.Tensor,
  cu_seqlens_q: torch.Tensor,
  cu_seqlens_k: torch.Tensor | None,
  max_seqlen_q: int,
  max_seqlen_k: int,
  *,
  dropout_p: float = 0.0,
  softmax_scale: float | None = None,
  causal: bool = False,
  enable_gqa: bool = False,
  return_lse: bool = False,
  **kwargs: object,
):
  """FFPA variable-length attention over packed sequences (FlashAttention's THD layout) — the reference's entry point under its name and signature
  (``src/ffpa_attn/ffpa_attn_interface.py:192-279``).  ``q`` is ``[T_q, H_q, D]``, ``k`` / ``v`` are ``[T_k, H_kv, D]``; ``cu_seqlens_q`` /
  ``cu_seqlens_k`` (int32 device tensors of length ``B + 1`` starting at 0; ``cu_seqlens_k=None`` = self-attention) mark the sequences.

  In the reference the CuTe-DSL backend ALONE serves this call (NVIDIA SM8x / SM90 / SM100; head dims 320 ... 1024).  Here it runs on the MI355X
  kernel of the dense path — ONE launch for the whole batch, the boundaries read on the device: nothing is copied to the host, the call never
  synchronises (the reference reads ``cu_seqlens`` back to check ``max_seqlen``) and captures into a HIP graph.  Same checks, same exception classes and
  texts (``varlen.py``); head dims: any up to 1024.

  ``causal`` = the reference's lower-right (tail-aligned) mask per sequence.  Rows without a visible key — an empty key sequence; the first
  ``N_q - N_k`` rows of a causal sequence with more queries than keys — come out as ``O = 0`` and ``LSE = -inf``
  (``tests/test_ffpa_cute_sm100.py:1117-1183``).  ``max_seqlen_q`` must be >= the longest query sequence (rows past it are not computed).
  ``dropout_p`` must be 0 and every FlashAttention-varlen extension (``window_size``, ``softcap``, ``seqused_k``, ``block_table`` ...) raises
  ``NotImplementedError``, as in the reference.  Returns ``out [T_q, H_q, D]`` — and ``lse [H_q, T_q]`` fp32 with ``return_lse=True``.  The LSE is
  differentiable; a loss that uses it routes the backward through the recompute path (``backward.py``) instead of aten's efficient-attention backward."""
  from .varlen import varlen_apply

  return varlen_apply(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, dropout_p=dropout_p, softmax_scale=softmax_scale,
                      causal=causal, enable_gqa=enable_gqa, return_lse=return_lse, kwargs=dict(kwargs))


# ----------------------------------------------------------------------------- the FP8 (e4m3 MFMA) forward, head dims 256 ... 512
_LOG2E = 1.4426950408889634


class AttnFp8(NamedTuple):
  """What ``quantize_attn_fp8`` returns: the scratch the kernels compute on (``q8`` / ``k8`` / ``v8t`` uint8 in fragment order, one row per tile; float32
  scales) and the same codes in the tensors' own layout (``*_codes [B, H, N, D]`` ``torch.float8_e4m3fn``)."""

  q8: torch.Tensor
  q_scale: torch.Tensor
  k8: torch.Tensor
  k_scale: torch.Tensor
  v8t: torch.Tensor
  v_scale: torch.Tensor
  q_codes: torch.Tensor
  k_codes: torch.Tensor
  v_codes: torch.Tensor
  k_mean: torch.Tensor


def _pow2_up_scale(amax: torch.Tensor) -> torch.Tensor:
  """``max(amax, 1e-4) / 448`` in float32, rounded UP to a power of two on its exponent bits (``quantize_index_rows``' rule)."""
  bits = (amax.clamp(min=1e-4) / 448).view(torch.int32)
  return ((bits & 0x7F800000) + ((bits & 0x007FFFFF) != 0).to(torch.int32) * 0x00800000).view(torch.float32)


def _pad_rows(x: torch.Tensor, block: int, dp: int) -> torch.Tensor:
  """``[B, H, N, D]`` -> ``[B, H, tiles, block, dp]``, zero rows / columns added."""
  B, H, N, D = x.shape
  tiles = -(-N // block)
  out = x.new_zeros((B, H, tiles * block, dp))
  out[:, :, :N, :D] = x
  return out.view(B, H, tiles, block, dp)


def _pack_fragments(codes: torch.Tensor, block: int) -> torch.Tensor:
  """Codes ``[B, H, N, D]`` (1 byte each) -> uint8 ``[B, H, tiles, block * DP]``: per tile, fragment (row block rb, column chunk c) of 2 KiB = plane h, lane
  16 g + r, byte e  <-  row 16 rb + r, column 128 c + 32 g + 16 h + e; rows past N and columns past D are zero codes."""
  B, H, N, D = codes.shape
  dp = -(-D // 128) * 128
  x = _pad_rows(codes.view(torch.uint8), block, dp)
  x = x.view(B, H, -1, block // 16, 16, dp // 128, 4, 2, 16)          # tile, rb, r, c, g, h, e
  return x.permute(0, 1, 2, 3, 5, 7, 6, 4, 8).reshape(B, H, -1, block * dp)  # tile, rb, c, h, g, r, e


def pack_attn_fp8_q(codes: torch.Tensor) -> torch.Tensor:
  """e4m3 codes of q ``[B, Hq, Nq, D]`` -> the kernel's ``q8`` scratch (tiles of FP8_BLOCK_ROWS rows)."""
  return _pack_fragments(codes, FP8_BLOCK_ROWS)


def pack_attn_fp8_k(codes: torch.Tensor) -> torch.Tensor:
  """e4m3 codes of k ``[B, Hkv, Nkv, D]`` -> the kernel's ``k8`` scratch (tiles of FP8_BLOCK_KEYS keys)."""
  return _pack_fragments(codes, FP8_BLOCK_KEYS)


def pack_attn_fp8_vt(codes: torch.Tensor) -> torch.Tensor:
  """e4m3 codes of v ``[B, Hkv, Nkv, D]`` -> the kernel's ``v8t`` scratch: per key tile, fragment db = channels 16 db + r, and contraction position
  ``p = 32 g + 16 h + e`` holds the tile's key ``16 ((p % 32) // 4) + 4 (p // 32) + p % 4`` — where the score accumulators leave that key's probability."""
  B, H, N, D = codes.shape
  x = _pad_rows(codes.view(torch.uint8), FP8_BLOCK_KEYS, D)
  x = x.view(B, H, -1, 2, 4, 4, 4, D // 16, 16)                        # tile, key = 16 (4 h + e4) + 4 g + i -> h, e4, g, i; then db, r
  return x.permute(0, 1, 2, 7, 3, 5, 8, 4, 6).reshape(B, H, -1, FP8_BLOCK_KEYS * D)  # tile, db, h, g, r, e4, i  (e = 4 e4 + i)


def quantize_attn_fp8(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, scale: "float | None" = None, smooth_k: bool = True) -> AttnFp8:
  """THE definition of what the FP8 forward computes on (plain torch, any device; ``ffpa_attn_fp8_quantize`` writes these bytes).  SageAttention-2 style::

      q:  x = float32(q) * float32(scale * log2(e));  one scale per tile of FP8_BLOCK_ROWS rows
      k:  x = float32(k) - mean  (smooth_k; softmax-invariant: no correction term);  one scale per tile of FP8_BLOCK_KEYS keys
          mean[b, h, d] = (sum over the key tiles, in tile order, of (the tile's keys added in key order)) / float32(Nkv), all in float32
      v:  x = float32(v);  one scale per (batch, KV head, channel) over all keys
      scale = max(amax |x|, 1e-4) / 448 rounded UP to a power of two;   code = rne_e4m3(clamp(x / scale, -448, +448))

  ``q ~ q_scale * q_codes`` in exp2-domain units, ``k - mean ~ k_scale * k_codes``, ``v ~ v_scale * v_codes``."""
  B, Hq, Nq, D = q.shape
  scale = D ** -0.5 if scale is None else float(scale)
  premul = torch.tensor(scale * _LOG2E, dtype=torch.float32, device=q.device)
  f8 = torch.float8_e4m3fn
  code = lambda x, s: (x / s).clamp(-448, 448).to(f8)

  qt = _pad_rows(q.float() * premul, FP8_BLOCK_ROWS, D)
  q_scale = _pow2_up_scale(qt.abs().amax(dim=(-1, -2)))
  q_codes = code(qt, q_scale[..., None, None]).flatten(2, 3)[:, :, :Nq]

  Nkv = k.size(2)
  kt = _pad_rows(k.float(), FP8_BLOCK_KEYS, D)
  part = torch.zeros_like(kt[:, :, :, 0])
  for j in range(FP8_BLOCK_KEYS):
    part = part + kt[:, :, :, j]
  mean = torch.zeros_like(part[:, :, 0])
  for t in range(part.size(2)):
    mean = mean + part[:, :, t]
  mean = mean / torch.tensor(float(Nkv), dtype=torch.float32, device=k.device) if smooth_k else torch.zeros_like(mean)
  kt = _pad_rows(k.float() - mean[:, :, None, :], FP8_BLOCK_KEYS, D)
  k_scale = _pow2_up_scale(kt.abs().amax(dim=(-1, -2)))
  k_codes = code(kt, k_scale[..., None, None]).flatten(2, 3)[:, :, :Nkv]

  vf = v.float()
  v_scale = _pow2_up_scale(vf.abs().amax(dim=2))
  v_codes = code(vf, v_scale[:, :, None, :])
  return AttnFp8(pack_attn_fp8_q(q_codes), q_scale, pack_attn_fp8_k(k_codes), k_scale, pack_attn_fp8_vt(v_codes), v_scale, q_codes, k_codes, v_codes, mean)


def _fp8_check(name: str, D: int, Hq: int, Hkv: int, enable_gqa: bool, attn_mask, dropout_p: float, return_lse: bool) -> None:
  if attn_mask is not None:
    raise NotImplementedError(f"{name}: attn_mask is not served by the FP8 forward (is_causal is); use ffpa_attn_func")
  if dropout_p != 0.0:
    raise NotImplementedError(f"{name}: dropout is not served by the FP8 forward; use ffpa_attn_func")
  if return_lse:
    raise NotImplementedError(f"{name}: the FP8 forward returns no LSE; use ffpa_attn_func")
  if D not in FP8_HEAD_DIMS:
    raise NotImplementedError(f"{name}: head dim {D} is not built; the FP8 forward serves {FP8_HEAD_DIMS} (D > 512 needs a split-D tile of its own)")
  if Hq % Hkv != 0:
    raise ValueError(f"query num_heads must be an integer multiple of key/value num_heads (GQA/MQA), got Nh_q={Hq}, Nh_kv={Hkv}")
  if not enable_gqa and Hq != Hkv:
    raise ValueError(f"enable_gqa=False but query num_heads ({Hq}) != key/value num_heads ({Hkv}). Set enable_gqa=True or use matching head counts.")


def ffpa_attn_fp8_codes(q8: torch.Tensor, q_scale: torch.Tensor, k8: torch.Tensor, k_scale: torch.Tensor, v8t: torch.Tensor, v_scale: torch.Tensor, *,
                        seqlen_q: int, seqlen_kv: int, is_causal: bool = False, out_dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
  """The FP8 attention kernel alone, on scratch in the layout of ``quantize_attn_fp8`` (``pack_attn_fp8_q`` / ``_k`` / ``_vt``) -> ``out [B, Hq, seqlen_q, D]``:

      s = q_scale[row tile] * k_scale[key tile] * (q8 . k8)      (exp2 domain: the softmax scale and log2(e) are in q)
      out = v_scale * sum_j 2^(s_j - max s) v8_j / sum_j 2^(s_j - max s)

  over the keys ``j < seqlen_kv`` and, with ``is_causal``, ``j <= row + seqlen_kv - seqlen_q``; a row that sees no key is 0.  A caller that keeps K / V
  quantised across calls (the denoising steps of a diffusion pipeline) quantises once and calls this."""
  if out_dtype not in (torch.bfloat16, torch.float16):
    raise TypeError(f"ffpa_attn_fp8_codes: out_dtype must be torch.bfloat16 or torch.float16, got {out_dtype}")
  if q8.dim() != 4 or k8.dim() != 4 or v_scale.dim() != 3:
    raise ValueError("ffpa_attn_fp8_codes: q8 / k8 / v8t must be [B, H, tiles, bytes] and v_scale [B, Hkv, D]")
  _fp8_check("ffpa_attn_fp8_codes", v_scale.size(-1), q8.size(1), k8.size(1), True, None, 0.0, False)
  return torch.ops.ffpa_attn._fp8_fwd_hip(q8, q_scale, k8, k_scale, v8t, v_scale, seqlen_q, seqlen_kv, bool(is_causal), out_dtype == torch.float16)


def ffpa_attn_fp8_func(query: torch.Tensor, key: torch.Tensor, value: torch.Tensor, *, is_causal: bool = False, scale: "float | None" = None,
                       enable_gqa: bool = False, smooth_k: bool = True, attn_mask=None, dropout_p: float = 0.0, return_lse: bool = False) -> torch.Tensor:
  """Attention forward with BOTH products on the e4m3 MFMA, head dims 256 / 320 / 384 / 448 / 512, inference only: the pre-pass (three HIP launches) quantises
  ``query [B, Hq, Nq, D]`` and ``key`` / ``value [B, Hkv, Nkv, D]`` (bf16 / fp16) as ``quantize_attn_fp8`` defines, one more launch computes
  ``out [B, Hq, Nq, D]`` in ``query``'s dtype.  Any ``Nq``, ``Nkv >= 1``; ``is_causal`` is tail-aligned as in ``ffpa_attn_func`` (key j visible to row i iff
  ``j <= i + Nkv - Nq``) and serves ``Nq > Nkv`` too: a row that sees no key is 0.  ``attn_mask``, dropout, an LSE and other head dims raise
  ``NotImplementedError``; so does a tensor that requires grad.  Nothing is read back to the host."""
  name = "ffpa_attn_fp8_func"
  for nm, t in (("query", query), ("key", key), ("value", value)):
    if not isinstance(t, torch.Tensor) or t.dim() != 4:
      raise ValueError(f"{name}: query/key/value must be 4-D [B, H, N, D] tensors")
  if query.dtype not in (torch.float16, torch.bfloat16) or key.dtype != query.dtype or value.dtype != query.dtype:
    raise TypeError(f"{name} only supports fp16/bf16 query/key/value of one dtype, got {query.dtype}, {key.dtype}, {value.dtype}")
  if key.shape != value.shape or key.size(0) != query.size(0) or key.size(3) != query.size(3):
    raise ValueError(f"{name}: key and value must share one shape [B, Hkv, Nkv, D], B and D query's; got {tuple(query.shape)}, {tuple(key.shape)}, {tuple(value.shape)}")
  _fp8_check(name, query.size(3), query.size(1), key.size(1), enable_gqa, attn_mask, dropout_p, return_lse)
  if query.size(2) < 1 or key.size(2) < 1:
    raise ValueError(f"{name}: Nq and Nkv must be at least 1")
  for nm, t in (("query", query), ("key", key), ("value", value)):
    if t.requires_grad and torch.is_grad_enabled():
      raise NotImplementedError(f"{name} is inference only: {nm} requires grad and there is no backward")
  if not query.is_cuda:
    raise NotImplementedError(f"{name} has no implementation for device '{query.device.type}' (the HIP kernel needs a GPU tensor)")
  scale = query.size(3) ** -0.5 if scale is None else float(scale)
  scratch = torch.ops.ffpa_attn._fp8_quantize_hip(query, key, value, scale * _LOG2E, bool(smooth_k))
  return torch.ops.ffpa_attn._fp8_fwd_hip(*scratch, query.size(2), key.size(2), bool(is_causal), query.dtype == torch.float16)
