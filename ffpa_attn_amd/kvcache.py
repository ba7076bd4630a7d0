"""``ffpa_attn_with_kvcache`` — FlashAttention's ``flash_attn_with_kvcache`` call (its signature and argument order) over a KV cache, contiguous or PAGED.

A serving engine keeps K and V either as one slab of fixed capacity per sequence (``k_cache [B, capacity, Hkv, D]``) or in a pool of fixed-size pages
(``k_cache [num_pages, page_size, Hkv, D]`` + ``block_table [B, pages_per_seq]``: vLLM, SGLang).  Both run as ONE launch of the packed-sequence kernel with the
lengths (``cache_seqlens``) read on the device: the contiguous cache through its ``seqused_k`` path (``hip.varlen_forward``), the paged cache through the paged
twin of that kernel (``ffpa_attn::_paged_fwd_hip`` -> ``ffpa_attn_varlen_paged_fwd``), which reads every K / V tile from its page — no gather into a contiguous
copy.  Nothing is read back to the host, so a call captures into a HIP graph, and replays follow ``cache_seqlens`` / ``block_table`` written in place.

With ``k`` / ``v`` (and optionally ``rotary_cos`` / ``rotary_sin``) the step's new keys are appended first, FlashAttention's decode call: ONE more launch on the
same stream in front of the attention launch (``ffpa_attn::_kvcache_append_hip`` -> ``ffpa_attn_kvcache_append``) writes key i of sequence b in place at
position ``cache_seqlens[b] + i`` (K rotated), the rotated copy of q, and the lengths ``cache_seqlens + Snew`` the attention launch reads.  Still no host
synchronisation: the two launches capture into one HIP graph.  ``cache_seqlens`` itself is not advanced (the caller does that, as with FlashAttention).

Local (sliding-window) attention has an entry of its own, ``ffpa_attn_with_kvcache_window`` (``window_size=(left, right)``, below): the KV tiles in front of
the window are not read.  ``ffpa_attn_with_kvcache`` itself keeps refusing ``window_size``.

Logit soft-capping (Gemma 2, Grok-1: scores ``softcap * tanh(softmax_scale * q.k / softcap)``) has an entry of its own as well,
``ffpa_attn_with_kvcache_softcap`` (``softcap=``, with or without ``window_size``, below): the cap is applied in the kernel, in front of the masks.  Every other
entry point keeps refusing ``softcap``.

An MLA latent cache — ONE cache whose rows are the keys and, in their first ``head_dim_v`` columns, the values (DeepSeek-V2 / V3 / R1, Kimi K2 in their
"absorbed" decode form) — has an entry of its own too, ``ffpa_attn_with_kvcache_mla`` (below): every latent row is fetched once, and the heads of a latent head are
packed into the rows of the tiles however many they are.  Sparse (top-k indexed) attention over that cache — every query token attends to the rows an
indexer picked for it (DeepSeek-V3.2) — is ``ffpa_attn_with_kvcache_mla_sparse`` (below): the rows are read where they lie.  An FP8 latent cache
(``torch.float8_e4m3fn`` codes under one per-tensor scale) is served by the ``_fp8`` twins of the latent calls:
``ffpa_attn_with_kvcache_mla_fp8``, ``ffpa_attn_varlen_with_kvcache_mla_fp8``, ``ffpa_attn_with_kvcache_mla_sparse_fp8``,
``ffpa_attn_with_kvcache_mla_tree_fp8`` and ``ffpa_attn_varlen_with_kvcache_mla_tree_fp8``.  The 656-byte FP8 rows in which DeepSeek-V3.2's cache is kept (e4m3
codes, four float32 scales per row, bf16 rotary columns) are served by the sparse call's ``ffpa_attn_with_kvcache_mla_sparse_ds``, written by
``store_latent_rows_ds`` and defined by ``pack_latent_rows_ds`` / ``unpack_latent_rows_ds``.
A batch whose sequences share their first latent rows — groups of consecutive sequences, prefix lengths and group boundaries on the device — is
``ffpa_attn_with_kvcache_mla_cascade`` (and its ``_fp8`` twin, at the end of this file): one plan launch, a prefix pass per group, a suffix pass and the merge.

Inference only: ``cache_batch_idx``, ``cache_leftpad`` and ALiBi have no kernel-side implementation here and raise
``NotImplementedError`` naming the option — as do ``k`` without ``v`` (or ``v`` without ``k``) and rotary tables without ``k`` / ``v`` or one without the other;
a tensor that requires grad raises (there is no backward).
"""

from __future__ import annotations

import torch

_DTYPES = (torch.float16, torch.bfloat16)


_UNIFORM, _RAGGED = "ffpa_attn_with_kvcache", "ffpa_attn_varlen_with_kvcache"  # the names the five uniform calls and the ragged call speak under


def _unsupported(cache_batch_idx, cache_leftpad, window_size, softcap, alibi_slopes) -> list[str]:
  """The options of ffpa_attn_with_kvcache's signature that no kernel serves, where the caller has set them."""
  names = [name for name, value in (("cache_batch_idx", cache_batch_idx), ("cache_leftpad", cache_leftpad)) if value is not None]
  if window_size is None or tuple(window_size) != (-1, -1):
    names.append("window_size")
  if softcap not in (None, 0, 0.0):
    names.append("softcap")
  if alibi_slopes is not None:
    names.append("alibi_slopes")
  return names


def _kv_check(name, q, k_cache, v_cache, k, v, rotary_cos, rotary_sin, cache_seqlens, block_table, softmax_scale, num_splits, unserved=(), ragged=None):
  """Every host-side check of the six calls (nothing read from the device, nothing launched), every rule written once, in the order the uniform calls (``ragged``
  None; ``unserved``: what ``_unsupported`` named) and the ragged call (``ragged = (cu_seqlens_q, max_seqlen_q, positions)``) make them
  -> ``(batch, capacity, the key lengths as an int32 [B] device tensor, softmax scale)``.  The two orders differ, and tests/golden/kv_front_calls.json holds both:
  the uniform calls test tensor and grad per tensor, ``cache_seqlens`` behind the caches and the grad of ``k`` / ``v`` with their other rules; the ragged call tests
  every tensor, then every grad, and ``cu_seqlens_q`` / ``max_seqlen_q`` / ``cache_seqlens`` in front of the caches."""
  from . import hip  # noqa: F401 (registers the ffpa_attn ops the step calls)

  append = k is not None and v is not None
  rotary = append and rotary_cos is not None and rotary_sin is not None
  bad = [nm for nm, t, ok in (("k", k, append), ("v", v, append), ("rotary_cos", rotary_cos, rotary), ("rotary_sin", rotary_sin, rotary)) if t is not None and not ok]
  if ragged is None:
    bad += unserved
    served = "; no leftpad, batch index, local window, softcap or ALiBi"
  else:
    cu_seqlens_q, max_seqlen_q, positions = ragged
    bad += ["positions"] if positions is not None and not rotary else []
    served = ", positions only with the rotary tables"
  if bad:
    raise NotImplementedError(f"{name} does not support: {', '.join(bad)} (k and v only together, rotary_cos and rotary_sin only together and with k / v{served})")
  caches = (("q", q), ("k_cache", k_cache), ("v_cache", v_cache))
  if ragged is None:  # (tensor and grad, tensor by tensor; k / v below)
    for nm, t in caches:
      if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: {nm} must be a tensor, got {type(t).__name__}")
      if t.requires_grad and torch.is_grad_enabled():
        raise NotImplementedError(f"{name} is inference only: {nm} requires grad and there is no backward")
  else:  # (every tensor, then every grad)
    for nm, t in caches + (("cu_seqlens_q", cu_seqlens_q), ("cache_seqlens", cache_seqlens)):
      if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: {nm} must be a tensor, got {type(t).__name__}")
    for nm, t in caches + (("k", k), ("v", v)):
      if isinstance(t, torch.Tensor) and t.requires_grad and torch.is_grad_enabled():
        raise NotImplementedError(f"{name} is inference only: {nm} requires grad and there is no backward")
  if q.dtype not in _DTYPES or k_cache.dtype != q.dtype or v_cache.dtype != q.dtype:
    raise TypeError(f"{name} only supports fp16/bf16 q/k_cache/v_cache of one dtype, got {q.dtype}, {k_cache.dtype}, {v_cache.dtype}")
  if q.dim() != (4 if ragged is None else 3) or k_cache.dim() != 4 or v_cache.dim() != 4:
    raise ValueError(f"{name}: q must be {'[B, Sq, Hq, D]' if ragged is None else 'packed [T, Hq, D]'} and k_cache / v_cache 4-D")
  if k_cache.shape != v_cache.shape:
    raise ValueError(f"{name}: k_cache {tuple(k_cache.shape)} and v_cache {tuple(v_cache.shape)} must share their shape")
  shape = q.shape  # (read once: every .size() is a call into torch)
  rows, Hq, D = shape[0], shape[-2], shape[-1]  # (rows: B of a uniform call, T of the ragged one)
  Hkv = k_cache.size(2)
  if k_cache.size(3) != D:
    raise ValueError(f"{name}: head dim of the cache ({k_cache.size(3)}) differs from q's ({D})")
  if D % 8 != 0 or D > 1024 or D <= 0:
    raise ValueError(f"{name}: head dim {D} is not a multiple of 8 in [8, 1024]")
  if Hkv == 0 or Hq % Hkv != 0:
    raise ValueError(f"{name}: query num_heads ({Hq}) must be a multiple of key/value num_heads ({Hkv})")
  if isinstance(num_splits, bool) or not isinstance(num_splits, int) or num_splits < 0:
    raise ValueError(f"{name}: num_splits must be a non-negative int, got {num_splits!r}")
  if ragged is None:
    B = rows
  else:
    if cu_seqlens_q.dtype != torch.int32:
      raise TypeError(f"{name}: cu_seqlens_q must be int32, got {cu_seqlens_q.dtype}")
    if cu_seqlens_q.dim() != 1 or cu_seqlens_q.numel() < 2 or cu_seqlens_q.stride(0) != 1 or cu_seqlens_q.device != q.device:
      raise ValueError(f"{name}: cu_seqlens_q must be a 1-D int32 tensor [batch + 1] of unit stride on q's device, got {tuple(cu_seqlens_q.shape)} on {cu_seqlens_q.device}")
    B = cu_seqlens_q.numel() - 1
    if isinstance(max_seqlen_q, bool) or not isinstance(max_seqlen_q, int) or max_seqlen_q < 0 or (rows > 0 and max_seqlen_q < 1):
      raise ValueError(f"{name}: max_seqlen_q must be a host int >= 1 (>= 0 without a token) that bounds every sequence's tokens, got {max_seqlen_q!r}")
    if cache_seqlens.dtype != torch.int32:
      raise TypeError(f"{name}: cache_seqlens must be int32, got {cache_seqlens.dtype}")
    if cache_seqlens.dim() != 1 or cache_seqlens.numel() != B or cache_seqlens.device != q.device:
      raise ValueError(f"{name}: cache_seqlens must be an int32 tensor [batch={B}] on q's device, got {tuple(cache_seqlens.shape)} on {cache_seqlens.device}")
  if block_table is not None:
    if not isinstance(block_table, torch.Tensor) or block_table.dtype != torch.int32 or block_table.dim() != 2 or block_table.size(0) != B:
      raise ValueError(f"{name}: block_table must be an int32 tensor [batch={B}, pages_per_seq]")
    if block_table.size(1) == 0:
      raise ValueError(f"{name}: block_table needs at least one page per sequence")
    page_size = k_cache.size(1)
    if page_size <= 0 or page_size % 64 != 0:
      raise ValueError(f"{name}: page_size ({page_size}) must be a positive multiple of 64 (smaller pages are not supported)")
    if block_table.device != q.device:
      raise ValueError(f"{name}: block_table must be on q's device, got {block_table.device} and {q.device}")
    capacity = block_table.size(1) * page_size
  else:
    if k_cache.size(0) != B:
      raise ValueError(f"{name}: k_cache [B, capacity, Hkv, D] must have {'q' if ragged is None else 'cu_seqlens_q'}'s batch ({B}), got {k_cache.size(0)}")
    capacity = k_cache.size(1)
  if k_cache.device != q.device or v_cache.device != q.device:
    raise ValueError(f"{name}: q / k_cache / v_cache must be on one device, got {q.device}, {k_cache.device}, {v_cache.device}")
  lens = cache_seqlens
  if ragged is None:  # (None, an int, or the tensor the ragged call has tested above)
    if cache_seqlens is None:
      lens = torch.full((B,), capacity, dtype=torch.int32, device=q.device)
    elif isinstance(cache_seqlens, int) and not isinstance(cache_seqlens, bool):
      if cache_seqlens < 0:
        raise ValueError(f"{name}: cache_seqlens must be non-negative, got {cache_seqlens}")
      lens = torch.full((B,), cache_seqlens, dtype=torch.int32, device=q.device)
    elif not isinstance(cache_seqlens, torch.Tensor):
      raise TypeError(f"{name}: cache_seqlens must be an int or an int32 tensor, got {type(cache_seqlens).__name__}")
    elif cache_seqlens.dtype != torch.int32 or cache_seqlens.dim() != 1 or cache_seqlens.numel() != B or cache_seqlens.device != q.device:
      raise ValueError(f"{name}: cache_seqlens must be an int or an int32 tensor [batch={B}] on q's device")
  scale = float(softmax_scale) if softmax_scale is not None else D ** -0.5
  if not append:
    return B, capacity, lens, scale
  if cache_seqlens is None:
    raise ValueError(f"{name}: cache_seqlens is required with k / v (it gives where the new keys go)")
  for nm, t in (("k", k), ("v", v)):
    if not isinstance(t, torch.Tensor):
      raise TypeError(f"{name}: {nm} must be a tensor, got {type(t).__name__}")
    if ragged is None and t.requires_grad and torch.is_grad_enabled():
      raise NotImplementedError(f"{name} is inference only: {nm} requires grad and there is no backward")
    if t.dtype != q.dtype:
      raise TypeError(f"{name}: {nm} must have the cache's dtype {q.dtype}, got {t.dtype}")
    if t.device != q.device:
      raise ValueError(f"{name}: {nm} must be on q's device, got {t.device} and {q.device}")
    new = t.shape
    if len(new) != len(shape) or new[0] != rows or new[-2] != Hkv or new[-1] != D:
      form = f"[B={B}, Snew, Hkv={Hkv}, D={D}]" if ragged is None else f"[T={rows}, Hkv={Hkv}, D={D}] (packed by cu_seqlens_q like q)"
      raise ValueError(f"{name}: {nm} must be {form}, got {tuple(new)}")
    if t.stride(-1) != 1:
      raise ValueError(f"{name}: {nm} must have a contiguous last dimension")
  if k.shape != v.shape:  # (Snew: a ragged call's k and v have no dimension left to differ in)
    raise ValueError(f"{name}: k {tuple(k.shape)} and v {tuple(v.shape)} must share their shape")
  if not rotary:
    return B, capacity, lens, scale
  for nm, t in (("rotary_cos", rotary_cos), ("rotary_sin", rotary_sin)):
    if not isinstance(t, torch.Tensor):
      raise TypeError(f"{name}: {nm} must be a tensor, got {type(t).__name__}")
    if t.dtype != q.dtype:
      raise TypeError(f"{name}: {nm} must have q's dtype {q.dtype}, got {t.dtype}")
    if t.device != q.device:
      raise ValueError(f"{name}: {nm} must be on q's device, got {t.device} and {q.device}")
    if t.dim() != 2 or not t.is_contiguous():
      raise ValueError(f"{name}: {nm} must be a contiguous [seqlen_ro, rotary_dim / 2] tensor, got {tuple(t.shape)}")
  if rotary_cos.shape != rotary_sin.shape:
    raise ValueError(f"{name}: rotary_cos {tuple(rotary_cos.shape)} and rotary_sin {tuple(rotary_sin.shape)} must share their shape")
  rotary_dim = 2 * rotary_cos.size(1)
  if rotary_dim == 0 or rotary_dim % 16 != 0 or rotary_dim > D:
    raise ValueError(f"{name}: rotary_dim ({rotary_dim}) must be a positive multiple of 16 and at most the head dim ({D})")
  if rotary_cos.size(0) < capacity:
    raise ValueError(f"{name}: rotary_cos / rotary_sin have {rotary_cos.size(0)} rows (seqlen_ro), fewer than the cache capacity {capacity}")
  if ragged is not None and positions is not None:
    if not isinstance(positions, torch.Tensor) or positions.dtype != torch.int32:
      raise TypeError(f"{name}: positions must be an int32 tensor, got {positions.dtype if isinstance(positions, torch.Tensor) else type(positions).__name__}")
    if positions.dim() != 1 or positions.numel() != rows or positions.stride(0) != 1 or positions.device != q.device:
      raise ValueError(f"{name}: positions must be int32 [T={rows}] of unit stride on q's device, got {tuple(positions.shape)} on {positions.device}")
  return B, capacity, lens, scale


# The step behind _kv_check.  ``family`` names the ONE attention launch, chosen by the entry point: ("plain",) — the paged op, or hip.varlen_forward over a contiguous
# cache —, ("tree", words), ("window", left, right) or ("softcap", cap, left, right); what follows the name are the op's own arguments, in its order.
def _kv_append(q, k_cache, v_cache, k, v, rotary_cos, rotary_sin, rotary_interleaved, causal, lens, block_table, ragged=None):
  """The prepare launch of a call with k / v: new keys into the cache (in place), rotated q, post-append lengths — read by the attention launch on the same stream
  -> (q to attend with, key lengths)."""
  if ragged is None:
    q_rot, lens = torch.ops.ffpa_attn._kvcache_append_hip(q, k_cache, v_cache, k, v, lens, block_table, rotary_cos, rotary_sin, bool(rotary_interleaved), bool(causal))
  else:
    q_rot, lens = torch.ops.ffpa_attn._kvcache_append_varlen_hip(q, k_cache, v_cache, k, v, ragged[0], lens, block_table, rotary_cos, rotary_sin, ragged[2],
                                                                 bool(rotary_interleaved), bool(causal))
  return (q_rot if rotary_cos is not None else q), lens


def _kv_view(k_cache, v_cache, B, capacity):
  """A CONTIGUOUS cache as the launch takes it -> (k, v, cu_seqlens_k): the packed call's seqused_k case — sequence b's keys are rows b * capacity ... of the cache
  viewed as [B * capacity, Hkv, D].  (Page pools go to the launch as they are, without a cu_seqlens_k.)"""
  Hkv, D = k_cache.size(2), k_cache.size(3)
  kp, vp = k_cache.reshape(B * capacity, Hkv, D), v_cache.reshape(B * capacity, Hkv, D)
  cu_k = torch.arange(0, (B + 1) * capacity, capacity, dtype=torch.int32, device=k_cache.device) if capacity > 0 else torch.zeros(B + 1, dtype=torch.int32, device=k_cache.device)
  return kp, vp, cu_k


def _kv_launch(family, qp, kp, vp, cu_q, cu_k, lens, block_table, max_seqlen_q, capacity, scale, causal, num_splits, return_lse=True):
  """The attention launch of ``family`` over packed q and ``_kv_view``'s caches -> packed ``(o [T, Hq, D], lse [Hq, T] | None)``."""
  kind, c = family[0], 1 if causal else 0
  if kind == "tree":
    return torch.ops.ffpa_attn._tree_fwd_hip(qp, kp, vp, cu_q, cu_k, lens, block_table, *family[1:], max_seqlen_q, capacity, scale, -1.0, num_splits)
  if kind == "window":
    return torch.ops.ffpa_attn._window_fwd_hip(qp, kp, vp, cu_q, cu_k, lens, block_table, *family[1:], max_seqlen_q, capacity, scale, c, -1.0, num_splits)
  if kind == "softcap":
    return torch.ops.ffpa_attn._softcap_fwd_hip(qp, kp, vp, cu_q, cu_k, lens, block_table, *family[1:], max_seqlen_q, capacity, scale, c, -1.0, num_splits)
  if block_table is not None:
    return torch.ops.ffpa_attn._paged_fwd_hip(qp, kp, vp, cu_q, lens, block_table, max_seqlen_q, capacity, scale, c, -1.0, num_splits)
  from . import hip

  return hip.varlen_forward(qp, kp, vp, cu_q, cu_k, max_seqlen_q, capacity, bool(causal), scale, return_lse=return_lse, seqused_k=lens, num_splits=num_splits)


def _kv_step(family, q, k_cache, v_cache, k, v, rotary_cos, rotary_sin, rotary_interleaved, lens, block_table, B, capacity, scale, causal, num_splits, return_lse,
             ragged=None):
  """The checked call's step: the append (``k`` / ``v``), q packed (a uniform call's as B sequences of Sq tokens), the cache view and the one attention launch of
  ``family`` -> packed ``(o [T, Hq, D], lse [Hq, T] | None)``."""
  if k is not None:
    q, lens = _kv_append(q, k_cache, v_cache, k, v, rotary_cos, rotary_sin, rotary_interleaved, causal, lens, block_table, ragged)
  if ragged is None:
    Sq, Hq, D = q.shape[1:]
    qp = q.reshape(B * Sq, Hq, D)
    cu_q = torch.arange(0, (B + 1) * Sq, Sq, dtype=torch.int32, device=q.device) if Sq > 0 else torch.zeros(B + 1, dtype=torch.int32, device=q.device)
  else:
    qp, cu_q, Sq = q, ragged[0], ragged[1]
  kp, vp, cu_k = (k_cache, v_cache, None) if block_table is not None else _kv_view(k_cache, v_cache, B, capacity)
  return _kv_launch(family, qp, kp, vp, cu_q, cu_k, lens, block_table, Sq, capacity, scale, causal, num_splits, return_lse)


def _kv_unpack(o, lse, q, return_lse):
  """A uniform call's returns: packed ``(o [B * Sq, Hq, D], lse [Hq, B * Sq])`` -> ``out [B, Sq, Hq, D]`` — and ``lse [B, Hq, Sq]``."""
  B, Sq, Hq, D = q.shape
  out = o.view(B, Sq, Hq, D)
  if not return_lse:
    return out
  return out, lse.view(Hq, B, Sq).permute(1, 0, 2).contiguous()


def ffpa_attn_with_kvcache(
  q: torch.Tensor,
  k_cache: torch.Tensor,
  v_cache: torch.Tensor,
  k: torch.Tensor | None = None,
  v: torch.Tensor | None = None,
  rotary_cos: torch.Tensor | None = None,
  rotary_sin: torch.Tensor | None = None,
  cache_seqlens: "int | torch.Tensor | None" = None,
  cache_batch_idx: torch.Tensor | None = None,
  cache_leftpad: torch.Tensor | None = None,
  block_table: torch.Tensor | None = None,
  softmax_scale: float | None = None,
  causal: bool = False,
  window_size: tuple = (-1, -1),
  softcap: float = 0.0,
  rotary_interleaved: bool = True,
  alibi_slopes: torch.Tensor | None = None,
  num_splits: int = 0,
  return_softmax_lse: bool = False,
):
  """Attention of ``q [B, Sq, Hq, D]`` against a KV cache: ``k_cache`` / ``v_cache [B, capacity, Hkv, D]`` without ``block_table``, or the page pools
  ``[num_pages, page_size, Hkv, D]`` with an int32 ``block_table [B, pages_per_seq]`` (``page_size`` a multiple of 64; key j of sequence b is row
  ``j % page_size`` of page ``block_table[b, j // page_size]``).  ``cache_seqlens``: an int, or an int32 ``[B]`` device tensor, of keys per sequence (None = the
  whole capacity).  ``causal`` is bottom-right aligned: query i of a sequence of ``Sq`` queries and ``L`` keys sees keys ``j <= i + L - Sq``.  GQA when
  ``Hq % Hkv == 0``.  ``num_splits``: 0 = the library decides, 1 = never split the keys, n = at most n ranges.  Returns ``out [B, Sq, Hq, D]`` — and the
  fp32 ``softmax_lse [B, Hq, Sq]`` with ``return_softmax_lse``.  Rows that see no key come out as 0 (LSE -inf).

  Layouts.  Strided views are read in place wherever the head dim has stride 1, every other stride is a multiple of 8 elements and the base is 16-byte
  aligned: K and V as the halves of one pool (``kv[:, 0]`` / ``kv[:, 1]`` of ``[num_pages, 2, page_size, Hkv, D]``, or ``kv[0]`` / ``kv[1]``), head-major pools
  viewed page-row-major, rows wider than D, q / k / v as slices of a fused QKV buffer; a ``block_table`` needs unit column stride (any row stride) and is copied
  otherwise, ``cache_seqlens`` is copied when strided.  A pool or cache outside that contract is copied for the attention launch (the right answer, at the
  price of the copy); the append writes in place and raises ``ValueError`` for it instead.  A CONTIGUOUS cache runs as ``[B * capacity, Hkv, D]``: one that is
  not viewable that way (``kv[:, 0]`` of ``[B, 2, capacity, Hkv, D]``, head-major slabs) is appended to in place and then copied for the attention launch
  — a documented copy, not an error; batch-padded (``cache[:B]``) and ``[2, B, ...]`` caches are viewable and are not copied.

  ``k`` / ``v [B, Snew, Hkv, D]`` (the cache's dtype, last dim contiguous; ``cache_seqlens`` required): key i of sequence b is written in place at position
  ``pos = cache_seqlens[b] + i`` (row ``pos`` of ``k_cache[b]``, or row ``pos % page_size`` of page ``block_table[b, pos // page_size]``; positions at or past the
  capacity are dropped, negative lengths act as 0), then attention runs over ``min(cache_seqlens[b] + Snew, capacity)`` keys.  ``cache_seqlens`` is not modified.
  Two sequences that append into one shared page race: the caller's problem, as with FlashAttention.  ``rotary_cos`` / ``rotary_sin [seqlen_ro, rotary_dim / 2]``
  (q's dtype, contiguous, ``rotary_dim`` a multiple of 16 <= D, ``seqlen_ro`` >= the capacity): the first ``rotary_dim`` dims of the new keys (stored rotated) and of
  q (a rotated copy attends; q is not modified) are rotated — key i at position ``cache_seqlens[b] + i``, query token i at ``cache_seqlens[b] + i`` when
  ``causal``, at ``cache_seqlens[b]`` otherwise; ``rotary_interleaved`` pairs dims (2j, 2j + 1), else (j, j + rotary_dim / 2) (GPT-NeoX).  V is never rotated."""
  unserved = _unsupported(cache_batch_idx, cache_leftpad, window_size, softcap, alibi_slopes)
  B, capacity, lens, scale = _kv_check(_UNIFORM, q, k_cache, v_cache, k, v, rotary_cos, rotary_sin, cache_seqlens, block_table, softmax_scale, num_splits, unserved)
  o, lse = _kv_step(("plain",), q, k_cache, v_cache, k, v, rotary_cos, rotary_sin, rotary_interleaved, lens, block_table, B, capacity, scale, causal, num_splits,
                    return_softmax_lse)
  return _kv_unpack(o, lse, q, return_softmax_lse)


# ---- tree-mask attention (the verification step of tree speculative decoding): ffpa_attn_with_kvcache_tree
_TREE_MAX_TOKENS = 64  # one 64-bit word per (sequence, token)


def pack_tree_mask(tree_mask: torch.Tensor) -> torch.Tensor:
  """The mask words the tree launch reads: ``tree_mask`` bool ``[Sq, Sq]`` (one tree for the batch) or ``[B, Sq, Sq]``, ``1 <= Sq <= 64`` -> int64 ``[1 | B, Sq]``
  with bit j of word ``[b, i]`` = ``tree_mask[b, i, j]`` (bit 63 is the int64's sign bit).  Torch ops on the mask's device, nothing read back to the host: a
  caller that replays a captured graph writes new words into the tensor it handed to ``ffpa_attn_with_kvcache_tree`` in place."""
  if not isinstance(tree_mask, torch.Tensor):
    raise TypeError(f"pack_tree_mask: tree_mask must be a tensor, got {type(tree_mask).__name__}")
  if tree_mask.dtype != torch.bool:
    raise TypeError(f"pack_tree_mask: tree_mask must be a torch.bool tensor, got {tree_mask.dtype}")
  if tree_mask.dim() not in (2, 3) or tree_mask.size(-1) != tree_mask.size(-2):
    raise ValueError(f"pack_tree_mask: tree_mask must be [Sq, Sq] or [B, Sq, Sq], got {tuple(tree_mask.shape)}")
  sq = tree_mask.size(-1)
  if not 1 <= sq <= _TREE_MAX_TOKENS:
    raise ValueError(f"pack_tree_mask: tree_mask holds Sq = {sq} tokens, outside [1, {_TREE_MAX_TOKENS}] (one 64-bit word per token)")
  m = tree_mask if tree_mask.dim() == 3 else tree_mask[None]
  bit = torch.ones((), dtype=torch.int64, device=m.device) << torch.arange(sq, dtype=torch.int64, device=m.device)  # (1 << 63 wraps to the sign bit)
  return (m.to(torch.int64) * bit).sum(dim=-1)  # (disjoint bits: the wrapping sum is the OR)


def _tree_words(tree_mask, B: int, Sq: int, device, name: str = "ffpa_attn_with_kvcache_tree", wide: bool = False) -> torch.Tensor:
  """``tree_mask`` of ffpa_attn_with_kvcache_tree checked against q's batch / tokens / device -> the int64 words ``[B | 1, Sq]``.  ``wide`` (the latent tree
  calls, under their ``name``): the mask may hold ``W`` tokens, ``Sq <= W <= 64`` -> ``[B | 1, W]``; a sequence of n tokens uses its top-left ``n x n``."""
  if not isinstance(tree_mask, torch.Tensor):
    raise TypeError(f"{name}: tree_mask must be a tensor, got {type(tree_mask).__name__}")
  if tree_mask.dtype not in (torch.bool, torch.int64):
    raise TypeError(f"{name}: tree_mask must be a torch.bool mask or int64 packed words (pack_tree_mask), got {tree_mask.dtype}")
  if not 1 <= Sq <= _TREE_MAX_TOKENS:
    raise ValueError(f"{name}: a tree_mask needs 1 <= Sq <= {_TREE_MAX_TOKENS} query tokens per sequence (one 64-bit word per token), got q with Sq = {Sq}")
  if tree_mask.device != device:
    raise ValueError(f"{name}: tree_mask must be on q's device, got {tree_mask.device} and {device}")
  if wide:
    W = tree_mask.size(-1) if tree_mask.dim() >= 2 else -1
    if tree_mask.dim() not in ((2,) if tree_mask.dtype == torch.int64 else (2, 3)) or not Sq <= W <= _TREE_MAX_TOKENS:
      raise ValueError(f"{name}: tree_mask must be bool [W, W] or [B={B}, W, W], or int64 words [B={B} or 1, W], with {Sq} <= W <= {_TREE_MAX_TOKENS} (the query "
                       f"tokens per sequence; one 64-bit word per token), got {tuple(tree_mask.shape)}")
    Sq = W
  if tree_mask.dtype == torch.int64:
    if tree_mask.dim() != 2 or tree_mask.size(0) not in (1, B) or tree_mask.size(1) != Sq:
      raise ValueError(f"{name}: a packed tree_mask must be int64 [B={B} or 1, Sq={Sq}], got {tuple(tree_mask.shape)}")
    return tree_mask
  if tree_mask.dim() not in (2, 3) or tuple(tree_mask.shape[-2:]) != (Sq, Sq) or (tree_mask.dim() == 3 and tree_mask.size(0) != B):
    raise ValueError(f"{name}: tree_mask must be bool [Sq={Sq}, Sq={Sq}] or [B={B}, Sq={Sq}, Sq={Sq}], got {tuple(tree_mask.shape)}")
  return pack_tree_mask(tree_mask)


def ffpa_attn_with_kvcache_tree(
  q: torch.Tensor,
  k_cache: torch.Tensor,
  v_cache: torch.Tensor,
  k: torch.Tensor | None = None,
  v: torch.Tensor | None = None,
  cache_seqlens: "int | torch.Tensor | None" = None,
  block_table: torch.Tensor | None = None,
  *,
  tree_mask: torch.Tensor,
  softmax_scale: float | None = None,
  num_splits: int = 0,
  return_softmax_lse: bool = False,
):
  """``ffpa_attn_with_kvcache`` under a TREE MASK: the verification step of tree speculative decoding (EAGLE, Medusa, SpecInfer; FlashInfer's ``custom_mask`` for
  that case).  The engine has appended — or appends here, with ``k`` / ``v`` — the ``Sq`` draft nodes of every sequence to its cache and calls attention once:
  node i sees the whole prefix and, among the ``Sq`` draft keys, what ``tree_mask`` says (its ancestors and itself, in a tree).  ONE attention launch of the
  same packed / paged kernel, the same plan as the causal call; no gather of the pages, no call per root-to-leaf path.

  Shapes, dtypes, layouts, strides, paged or contiguous caches, GQA, ``num_splits`` and the returns are ``ffpa_attn_with_kvcache``'s.  ``tree_mask``: a
  ``torch.bool`` tensor on q's device, ``[Sq, Sq]`` (one tree for the batch) or ``[B, Sq, Sq]``, ``1 <= Sq <= 64`` — or the int64 words ``[B | 1, Sq]``
  ``pack_tree_mask`` makes of one (bit j of word ``[b, i]`` = ``tree_mask[b, i, j]``).  With ``L_b`` the keys attention runs over (``min(cache_seqlens[b] + Snew,
  capacity)`` with ``k`` / ``v``, else ``cache_seqlens[b]`` clamped to the capacity), query token i of sequence b sees

  * key ``p`` for every ``p < L_b - Sq`` (the prefix), and
  * key ``L_b - Sq + j`` iff ``tree_mask[b, i, j]``; draft positions below 0 (``L_b < Sq``) do not exist.

  The mask is arbitrary: a False diagonal and "sees a later node" are legal; ``tril(ones)`` is the causal call and all ones the non-causal one, to the bit.  A
  row that sees no key returns O = 0, LSE = -inf.  ``k`` / ``v`` append exactly as in ``ffpa_attn_with_kvcache`` (key i at ``cache_seqlens[b] + i``: the same
  launch).  There is no ``rotary_cos`` / ``rotary_sin`` here: a tree node's position is its DEPTH, not its index among the new keys, and the append kernel has
  no per-token positions — rotate q and the draft keys before the call.  Nothing is read back to the host: the call captures into one HIP graph, and a replay
  follows ``cache_seqlens``, ``block_table`` and the mask written in place — a bool mask is packed inside the graph; hand over packed words to write words.
  Inference only: a tensor that requires grad raises ``NotImplementedError``."""
  B, capacity, lens, scale = _kv_check(_UNIFORM, q, k_cache, v_cache, k, v, None, None, cache_seqlens, block_table, softmax_scale, num_splits)
  if isinstance(tree_mask, torch.Tensor) and tree_mask.requires_grad and torch.is_grad_enabled():
    raise NotImplementedError("ffpa_attn_with_kvcache is inference only: tree_mask requires grad and there is no backward")
  words = _tree_words(tree_mask, B, q.size(1), q.device)
  o, lse = _kv_step(("tree", words), q, k_cache, v_cache, k, v, None, None, True, lens, block_table, B, capacity, scale, False, num_splits, True)
  return _kv_unpack(o, lse, q, return_softmax_lse)


# ---- sliding-window (local) attention: ffpa_attn_with_kvcache_window
def _window_pair(window_size) -> "tuple[int, int]":
  """``window_size`` of ffpa_attn_with_kvcache_window -> (left, right): a pair of ints >= -1."""
  name = "ffpa_attn_with_kvcache_window"
  if not isinstance(window_size, (tuple, list)) or len(window_size) != 2:
    raise TypeError(f"{name}: window_size must be a pair of ints (left, right), got {window_size!r}")
  for x in window_size:
    if isinstance(x, bool) or not isinstance(x, int):
      raise TypeError(f"{name}: window_size must be a pair of ints (left, right), got {window_size!r}")
  left, right = int(window_size[0]), int(window_size[1])
  if left < -1 or right < -1:
    raise ValueError(f"{name}: window_size = ({left}, {right}): each side must be >= -1 (-1 = unbounded)")
  return min(left, 0x7FFFFFFF), min(right, 0x7FFFFFFF)


def _window_arg(window_size) -> "tuple[int, int]":
  """``window_size`` as the window, softcap and ragged calls take it: ``_window_pair``, with None refused by the same TypeError."""
  if window_size is None:
    raise TypeError("ffpa_attn_with_kvcache_window: window_size must be a pair of ints (left, right), got None")
  return _window_pair(window_size)


def _softcap_arg(softcap) -> float:
  """``softcap`` as the softcap and ragged calls take it: a real number (not a bool), finite and >= 0 (0 = off)."""
  if isinstance(softcap, bool) or not isinstance(softcap, (int, float)):
    raise TypeError(f"ffpa_attn_with_kvcache_softcap: softcap must be a real number, got {softcap!r}")
  softcap = float(softcap)
  if not 0.0 <= softcap < float("inf"):  # (NaN fails both comparisons)
    raise ValueError(f"ffpa_attn_with_kvcache_softcap: softcap = {softcap} must be finite and >= 0 (0 = off)")
  return softcap


def ffpa_attn_with_kvcache_window(
  q: torch.Tensor,
  k_cache: torch.Tensor,
  v_cache: torch.Tensor,
  k: torch.Tensor | None = None,
  v: torch.Tensor | None = None,
  rotary_cos: torch.Tensor | None = None,
  rotary_sin: torch.Tensor | None = None,
  cache_seqlens: "int | torch.Tensor | None" = None,
  block_table: torch.Tensor | None = None,
  *,
  window_size: tuple,
  softmax_scale: float | None = None,
  causal: bool = False,
  rotary_interleaved: bool = True,
  num_splits: int = 0,
  return_softmax_lse: bool = False,
):
  """``ffpa_attn_with_kvcache`` under a SLIDING WINDOW — the local attention layers of Mistral, Gemma 2 / 3, Phi-3 and the long-context hybrids; FlashAttention's
  ``window_size``.  ONE attention launch of the packed / paged kernel's window build: a row tile walks only the KV tiles between the left bound of its first token
  and the right bound of its last one — the tiles, and the pages, in front of the window are never read, which on a decode step is the whole cost —, and the launch
  plan (KV splits, the non-temporal fetch) is made for the window's keys, not the cache's capacity.

  Shapes, dtypes, layouts, strides, paged or contiguous caches, GQA, the append of ``k`` / ``v`` with ``rotary_cos`` / ``rotary_sin``, ``num_splits`` and the returns
  are ``ffpa_attn_with_kvcache``'s.  ``window_size = (left, right)``, ints >= -1 with -1 = unbounded on that side (``TypeError`` for anything but a pair of ints,
  ``ValueError`` below -1).  With ``L_b`` the keys attention runs over (``min(cache_seqlens[b] + Snew, capacity)`` with ``k`` / ``v``, else ``cache_seqlens[b]``
  clamped to the capacity) and ``pos_i = i + L_b - Sq`` the position of query token i (bottom-right aligned), token i sees key j iff

  * ``0 <= j < L_b``,
  * ``left < 0 or j >= pos_i - left``,
  * ``right < 0 or j <= pos_i + right``.

  ``causal=True`` means ``right = 0`` whatever ``right`` was given.  ``(-1, -1)`` is ``ffpa_attn_with_kvcache`` and ``(-1, 0)`` its causal call, to the bit (bf16).
  A row that sees no key returns O = 0, LSE = -inf.  Nothing is read back to the host: the call captures into one HIP graph, and a replay follows
  ``cache_seqlens`` / ``block_table`` written in place.  Inference only: a tensor that requires grad raises ``NotImplementedError``."""
  left, right = _window_arg(window_size)
  B, capacity, lens, scale = _kv_check(_UNIFORM, q, k_cache, v_cache, k, v, rotary_cos, rotary_sin, cache_seqlens, block_table, softmax_scale, num_splits)
  o, lse = _kv_step(("window", left, right), q, k_cache, v_cache, k, v, rotary_cos, rotary_sin, rotary_interleaved, lens, block_table, B, capacity, scale, causal,
                    num_splits, True)
  return _kv_unpack(o, lse, q, return_softmax_lse)


# ---- logit soft-capping, with or without a sliding window: ffpa_attn_with_kvcache_softcap
def ffpa_attn_with_kvcache_softcap(
  q: torch.Tensor,
  k_cache: torch.Tensor,
  v_cache: torch.Tensor,
  k: torch.Tensor | None = None,
  v: torch.Tensor | None = None,
  rotary_cos: torch.Tensor | None = None,
  rotary_sin: torch.Tensor | None = None,
  cache_seqlens: "int | torch.Tensor | None" = None,
  block_table: torch.Tensor | None = None,
  *,
  softcap: float,
  window_size: tuple = (-1, -1),
  softmax_scale: float | None = None,
  causal: bool = False,
  rotary_interleaved: bool = True,
  num_splits: int = 0,
  return_softmax_lse: bool = False,
):
  """``ffpa_attn_with_kvcache_window`` with LOGIT SOFT-CAPPING — FlashAttention's ``softcap``; Gemma 2 caps its attention logits at 50 in every layer (half of
  them under a 4096-key window, half of them global), Grok-1 at 30.  With ``c = softcap > 0``

      ``score(i, j) = c * tanh(softmax_scale * q_i . k_j / c)``;

  the mask — the key length, the causal edge, the window's edges — is applied to the capped score (a hidden key has weight 0), and the softmax, O and the LSE
  (natural log) are taken over the capped scores.  ONE attention launch of the packed / paged kernel's soft-capping build (the window build with the cap on: one
  exp2 and one rcp per score, absolute tanh error <= 2^-21): ``window_size = (-1, -1)``, the default, walks the plain call's tiles, so the same kernel serves the
  global and the local layers.

  Shapes, dtypes, layouts, strides, paged or contiguous caches, GQA, the append of ``k`` / ``v`` with ``rotary_cos`` / ``rotary_sin``, ``window_size`` and its
  errors, ``causal``, ``num_splits`` and the returns are ``ffpa_attn_with_kvcache_window``'s; a row that sees no key returns O = 0, LSE = -inf.  ``softcap`` must
  be a real number (``TypeError`` otherwise, for a bool too), not negative, NaN or inf (``ValueError``); ``softcap == 0`` means "off" and forwards to
  ``ffpa_attn_with_kvcache_window``: the same launch, the same bits.  Nothing is read back to the host: the call captures into one HIP graph, and a replay follows
  ``cache_seqlens`` / ``block_table`` written in place.  Inference only: a tensor that requires grad raises ``NotImplementedError``."""
  softcap = _softcap_arg(softcap)
  left, right = _window_arg(window_size)
  if softcap == 0.0:
    return ffpa_attn_with_kvcache_window(q, k_cache, v_cache, k, v, rotary_cos, rotary_sin, cache_seqlens, block_table, window_size=(left, right),
                                         softmax_scale=softmax_scale, causal=causal, rotary_interleaved=rotary_interleaved, num_splits=num_splits,
                                         return_softmax_lse=return_softmax_lse)
  B, capacity, lens, scale = _kv_check(_UNIFORM, q, k_cache, v_cache, k, v, rotary_cos, rotary_sin, cache_seqlens, block_table, softmax_scale, num_splits)
  o, lse = _kv_step(("softcap", softcap, left, right), q, k_cache, v_cache, k, v, rotary_cos, rotary_sin, rotary_interleaved, lens, block_table, B, capacity, scale,
                    causal, num_splits, True)
  return _kv_unpack(o, lse, q, return_softmax_lse)


# ---- MLA latent-cache attention (DeepSeek-V2 / V3 / R1, Kimi K2 in their "absorbed" decode form): ffpa_attn_with_kvcache_mla
_MLA_REQUIRED = object()
_MLA_IDENTITY: "dict[tuple, torch.Tensor]" = {}


def _mla_identity_table(B: int, device) -> torch.Tensor:
  """The block table of a contiguous latent cache — one page per sequence, page b = slab b — made on the device once per (B, device)."""
  key = (B, device.type, device.index)
  t = _MLA_IDENTITY.get(key)
  if t is None:
    if len(_MLA_IDENTITY) >= 64:
      _MLA_IDENTITY.clear()
    t = _MLA_IDENTITY[key] = torch.arange(B, dtype=torch.int32, device=device).view(B, 1)
  return t


def _mla_check(name, q, kv_cache, head_dim_v, kv, cache_seqlens, block_table, softmax_scale, num_splits, fp8=False, ragged=None):
  """The argument checks of the six latent calls under their own ``name``, every rule written once, in the order the uniform calls (``ragged`` None) and the
  ragged calls (``ragged = (cu_seqlens_q, max_seqlen_q)``) make them -> ``(capacity, cache_seqlens as an int32 [B] device tensor)``.  The two orders differ, and
  tests/golden/mla_front_calls.json holds both: the uniform calls test tensor and grad per tensor and ``cache_seqlens`` behind the pool; the ragged ones test
  every tensor, then every grad, and ``cache_seqlens`` in front of the pool.  ``fp8``: the cache is ``torch.float8_e4m3fn`` (the ``_fp8`` calls)."""
  if softmax_scale is _MLA_REQUIRED or softmax_scale is None:
    raise TypeError(f"{name}: softmax_scale is required — an MLA model scales by 1 / sqrt(qk_nope_head_dim + qk_rope_head_dim) (x its YaRN factor), which is not "
                    "1 / sqrt(D) of the 576-wide absorbed head: there is no right default")
  if isinstance(softmax_scale, bool) or not isinstance(softmax_scale, (int, float)):
    raise TypeError(f"{name}: softmax_scale must be a real number, got {softmax_scale!r}")
  named = (("q", q), ("kv_cache", kv_cache), ("kv", kv)) if kv is not None else (("q", q), ("kv_cache", kv_cache))
  if ragged is None:  # (tensor and grad, tensor by tensor)
    for nm, t in named:
      if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: {nm} must be a tensor, got {type(t).__name__}")
      if t.requires_grad and torch.is_grad_enabled():
        raise NotImplementedError(f"{name} is inference only: {nm} requires grad and there is no backward")
  else:  # (every tensor, then every grad)
    cu_seqlens_q, max_seqlen_q = ragged
    for nm, t in (("q", q), ("kv_cache", kv_cache), ("cu_seqlens_q", cu_seqlens_q), ("cache_seqlens", cache_seqlens)) + named[2:]:
      if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: {nm} must be a tensor, got {type(t).__name__}")
    for nm, t in named:
      if t.requires_grad and torch.is_grad_enabled():
        raise NotImplementedError(f"{name} is inference only: {nm} requires grad and there is no backward")
  if fp8:
    if q.dtype not in _DTYPES or kv_cache.dtype != torch.float8_e4m3fn:
      raise TypeError(f"{name} only supports fp16/bf16 q over a torch.float8_e4m3fn kv_cache — OCP e4m3 is the chip's FP8 format; float8_e4m3fnuz and the e5m2 "
                      f"formats are not served —, got {q.dtype}, {kv_cache.dtype}")
  elif q.dtype not in _DTYPES or kv_cache.dtype != q.dtype:
    raise TypeError(f"{name} only supports fp16/bf16 q/kv_cache of one dtype, got {q.dtype}, {kv_cache.dtype}")
  if q.dim() != (4 if ragged is None else 3) or kv_cache.dim() != 4:
    raise ValueError(f"{name}: q must be {'[B, Sq, Hq, D]' if ragged is None else 'packed [T, Hq, D]'} and kv_cache 4-D")
  shape, pool = q.shape, kv_cache.shape  # (read once: every .size() is a call into torch)
  rows, Hq, D = shape[0], shape[-2], shape[-1]  # (rows: B of a uniform call, T of a ragged one)
  Hkv = pool[2]
  if pool[3] != D:
    raise ValueError(f"{name}: head dim of the cache ({pool[3]}) differs from q's ({D})")
  if isinstance(head_dim_v, bool) or not isinstance(head_dim_v, int):
    raise TypeError(f"{name}: head_dim_v must be an int, got {head_dim_v!r}")
  if D % 64 != 0 or head_dim_v <= 0 or head_dim_v % 64 != 0 or head_dim_v > D:
    raise ValueError(f"{name}: (D, head_dim_v) = ({D}, {head_dim_v}): both must be multiples of 64 with 0 < head_dim_v <= D")
  from .hip import MLA_BUILDS

  if (D, head_dim_v) not in MLA_BUILDS:
    raise NotImplementedError(f"{name}: (D, head_dim_v) = ({D}, {head_dim_v}) is not built (built: {', '.join(map(str, MLA_BUILDS))})")
  if Hkv == 0 or Hq % Hkv != 0:
    raise ValueError(f"{name}: query num_heads ({Hq}) must be a multiple of the latent num_heads ({Hkv})")
  if isinstance(num_splits, bool) or not isinstance(num_splits, int) or num_splits < 0:
    raise ValueError(f"{name}: num_splits must be a non-negative int, got {num_splits!r}")
  if kv_cache.device != q.device:
    raise ValueError(f"{name}: q / kv_cache must be on one device, got {q.device}, {kv_cache.device}")
  if ragged is None:
    B = rows
  else:
    if cu_seqlens_q.dtype != torch.int32:
      raise TypeError(f"{name}: cu_seqlens_q must be int32, got {cu_seqlens_q.dtype}")
    if cu_seqlens_q.dim() != 1 or cu_seqlens_q.numel() < 2 or cu_seqlens_q.stride(0) != 1 or cu_seqlens_q.device != q.device:
      raise ValueError(f"{name}: cu_seqlens_q must be a 1-D int32 tensor [batch + 1] of unit stride on q's device, got {tuple(cu_seqlens_q.shape)} on {cu_seqlens_q.device}")
    B = cu_seqlens_q.numel() - 1
    if isinstance(max_seqlen_q, bool) or not isinstance(max_seqlen_q, int) or max_seqlen_q < 0 or (rows > 0 and max_seqlen_q < 1):
      raise ValueError(f"{name}: max_seqlen_q must be a host int >= 1 (>= 0 without a token) that bounds every sequence's tokens, got {max_seqlen_q!r}")
    if cache_seqlens.dtype != torch.int32:
      raise TypeError(f"{name}: cache_seqlens must be int32, got {cache_seqlens.dtype}")
    if cache_seqlens.dim() != 1 or cache_seqlens.numel() != B or cache_seqlens.device != q.device:
      raise ValueError(f"{name}: cache_seqlens must be an int32 tensor [batch={B}] on q's device, got {tuple(cache_seqlens.shape)} on {cache_seqlens.device}")
  if block_table is not None:
    if not isinstance(block_table, torch.Tensor) or block_table.dtype != torch.int32 or block_table.dim() != 2 or block_table.size(0) != B:
      raise ValueError(f"{name}: block_table must be an int32 tensor [batch={B}, pages_per_seq]")
    if block_table.size(1) == 0:
      raise ValueError(f"{name}: block_table needs at least one page per sequence")
    page_size = pool[1]
    if page_size <= 0 or page_size % 64 != 0:
      raise ValueError(f"{name}: page_size ({page_size}) must be a positive multiple of 64 (smaller pages are not supported)")
    if block_table.device != q.device:
      raise ValueError(f"{name}: block_table must be on q's device, got {block_table.device} and {q.device}")
    capacity = block_table.size(1) * page_size
  else:
    if pool[0] != B:
      raise ValueError(f"{name}: kv_cache [B, capacity, Hkv, D] must have {'q' if ragged is None else 'cu_seqlens_q'}'s batch ({B}), got {pool[0]}")
    capacity = pool[1]
    if capacity <= 0 or capacity % 64 != 0:
      raise ValueError(f"{name}: a contiguous cache runs as a pool of one page per sequence: its capacity ({capacity}) must be a positive multiple of 64")
  if ragged is None:  # (an int, or the tensor the ragged calls have tested above)
    if isinstance(cache_seqlens, int) and not isinstance(cache_seqlens, bool):
      if cache_seqlens < 0:
        raise ValueError(f"{name}: cache_seqlens must be non-negative, got {cache_seqlens}")
      cache_seqlens = torch.full((B,), cache_seqlens, dtype=torch.int32, device=q.device)
    elif not isinstance(cache_seqlens, torch.Tensor):
      raise TypeError(f"{name}: cache_seqlens must be an int or an int32 tensor, got {type(cache_seqlens).__name__}")
    elif cache_seqlens.dtype != torch.int32 or cache_seqlens.dim() != 1 or cache_seqlens.numel() != B or cache_seqlens.device != q.device:
      raise ValueError(f"{name}: cache_seqlens must be an int or an int32 tensor [batch={B}] on q's device")
  if kv is not None:
    if kv.dtype != q.dtype:
      raise TypeError(f"{name}: kv must have {'q' if fp8 else 'the cache'}'s dtype {q.dtype}, got {kv.dtype}")
    if kv.device != q.device:
      raise ValueError(f"{name}: kv must be on q's device, got {kv.device} and {q.device}")
    new = kv.shape
    if len(new) != len(shape) or new[0] != rows or new[-2] != Hkv or new[-1] != D:
      form = f"[B={B}, Snew, Hkv={Hkv}, D={D}]" if ragged is None else f"[T={rows}, Hkv={Hkv}, D={D}] (packed by cu_seqlens_q like q)"
      raise ValueError(f"{name}: kv must be {form}, got {tuple(new)}")
    if kv.stride(-1) != 1:
      raise ValueError(f"{name}: kv must have a contiguous last dimension")
  return capacity, cache_seqlens


# The step behind _mla_check, once per kind.  ``op`` names the attention op: "mla" is ffpa_attn::_mla_fwd_hip; "fp8" its FP8 twin, with ``extra`` the kv_scale; "tree"
# its tree-mask twin, with ``extra`` the caller's tree_mask — checked here, behind the empty returns that never look at it — and no causal flag.  The ops are
# registered: _mla_check has imported .hip.  "tree_fp8" is the tree twin over an FP8 pool: ``extra`` is ``(tree_mask, kv_scale)``, the mask checked where "tree"
# checks it, the rows of ``kv`` quantised by the appends "fp8" uses.
def _mla_step(name, op, extra, q, kv_cache, head_dim_v, kv, lens, block_table, capacity, softmax_scale, causal, num_splits, return_softmax_lse):
  """The uniform step: append (``kv``) + attention in ONE call of the attention op, q as a packed batch of B sequences of Sq tokens."""
  B, Sq, Hq, D = q.shape
  if B == 0 or Sq == 0:
    out = q.new_zeros((B, Sq, Hq, head_dim_v))
    return (out, q.new_full((B, Hq, Sq), float("-inf"), dtype=torch.float32)) if return_softmax_lse else out
  if op == "tree":
    extra = _tree_words(extra, B, Sq, q.device, name, wide=True)  # (from here on `extra` is the packed words the tree op takes, no longer the caller's mask)
  elif op == "tree_fp8":
    extra = (_tree_words(extra[0], B, Sq, q.device, name, wide=True), extra[1])
  table = block_table if block_table is not None else _mla_identity_table(B, q.device)
  qp = q.reshape(B * Sq, Hq, D)
  cu_q = torch.arange(0, (B + 1) * Sq, Sq, dtype=torch.int32, device=q.device)
  kv_new = kv if kv is not None and kv.size(1) > 0 else None
  seqused = torch.empty((B,), dtype=torch.int32, device=q.device) if kv_new is not None else lens
  before = lens if kv_new is not None else None
  if op == "tree":
    o, lse = torch.ops.ffpa_attn._mla_tree_fwd_hip(qp, kv_cache, head_dim_v, cu_q, seqused, table, extra, kv_new, before, Sq, capacity, float(softmax_scale), num_splits)
  elif op == "tree_fp8":
    o, lse = torch.ops.ffpa_attn._mla_tree_fp8_fwd_hip(qp, kv_cache, head_dim_v, extra[1], cu_q, seqused, table, extra[0], kv_new, before, Sq, capacity,
                                                       float(softmax_scale), num_splits)
  elif op == "fp8":
    o, lse = torch.ops.ffpa_attn._mla_fp8_fwd_hip(qp, kv_cache, head_dim_v, extra, cu_q, seqused, table, kv_new, before, Sq, capacity, float(softmax_scale),
                                                  1 if causal else 0, num_splits)
  else:
    o, lse = torch.ops.ffpa_attn._mla_fwd_hip(qp, kv_cache, head_dim_v, cu_q, seqused, table, kv_new, before, Sq, capacity, float(softmax_scale), 1 if causal else 0,
                                              num_splits)
  out = o.view(B, Sq, Hq, head_dim_v)
  if not return_softmax_lse:
    return out
  return out, lse.view(Hq, B, Sq).permute(1, 0, 2).contiguous()


def _mla_step_varlen(name, op, extra, q, kv_cache, head_dim_v, cu_seqlens_q, max_seqlen_q, kv, lens, block_table, capacity, softmax_scale, causal, num_splits,
                     return_softmax_lse):
  """The ragged step: the per-token append launch (``kv``), then the attention launch over the lengths it returns."""
  T, Hq, D = q.shape
  B = cu_seqlens_q.numel() - 1
  if T == 0:
    out = q.new_empty((0, Hq, head_dim_v))
    return (out, torch.empty((Hq, 0), dtype=torch.float32, device=q.device)) if return_softmax_lse else out
  if op == "tree":
    extra = _tree_words(extra, B, max_seqlen_q, q.device, name, wide=True)  # (from here on `extra` is the packed words the tree op takes, no longer the caller's mask)
  elif op == "tree_fp8":
    extra = (_tree_words(extra[0], B, max_seqlen_q, q.device, name, wide=True), extra[1])
  table = block_table if block_table is not None else _mla_identity_table(B, q.device)
  seqused = lens
  if kv is not None:
    # the prepare launch: the step's latent rows into the cache (in place) and the post-append lengths — read by the attention launch below on the same stream
    if op in ("fp8", "tree_fp8"):
      seqused = torch.ops.ffpa_attn._mla_fp8_append_varlen_hip(kv_cache, kv, extra if op == "fp8" else extra[1], cu_seqlens_q, lens, table)
    else:
      seqused = torch.ops.ffpa_attn._mla_append_varlen_hip(kv_cache, kv, cu_seqlens_q, lens, table)
  if op == "tree":
    o, lse = torch.ops.ffpa_attn._mla_tree_fwd_hip(q, kv_cache, head_dim_v, cu_seqlens_q, seqused, table, extra, None, None, max_seqlen_q, capacity,
                                                   float(softmax_scale), num_splits)
  elif op == "tree_fp8":
    o, lse = torch.ops.ffpa_attn._mla_tree_fp8_fwd_hip(q, kv_cache, head_dim_v, extra[1], cu_seqlens_q, seqused, table, extra[0], None, None, max_seqlen_q, capacity,
                                                       float(softmax_scale), num_splits)
  elif op == "fp8":
    o, lse = torch.ops.ffpa_attn._mla_fp8_fwd_hip(q, kv_cache, head_dim_v, extra, cu_seqlens_q, seqused, table, None, None, max_seqlen_q, capacity,
                                                  float(softmax_scale), 1 if causal else 0, num_splits)
  else:
    o, lse = torch.ops.ffpa_attn._mla_fwd_hip(q, kv_cache, head_dim_v, cu_seqlens_q, seqused, table, None, None, max_seqlen_q, capacity, float(softmax_scale),
                                              1 if causal else 0, num_splits)
  return (o, lse) if return_softmax_lse else o


def ffpa_attn_with_kvcache_mla(
  q: torch.Tensor,
  kv_cache: torch.Tensor,
  head_dim_v: int,
  *,
  kv: torch.Tensor | None = None,
  cache_seqlens: "int | torch.Tensor",
  block_table: torch.Tensor | None = None,
  softmax_scale: float = _MLA_REQUIRED,
  causal: bool = False,
  num_splits: int = 0,
  return_softmax_lse: bool = False,
  **unsupported,
):
  """Attention of ``q [B, Sq, Hq, D]`` over an MLA LATENT cache: ONE cache holds, per KV head h, rows whose ``D`` columns are the keys
  (``kv_cache[..., h, :]``) and whose first ``head_dim_v`` columns are the values (``kv_cache[..., h, :head_dim_v]``) — multi-head latent attention in its
  "absorbed" decode form, where every query head (D = 576: a 512-wide compressed latent + 64 rotary columns) attends to one latent head.  Returns
  ``out [B, Sq, Hq, head_dim_v]`` and, with ``return_softmax_lse``, the fp32 ``lse [B, Hq, Sq]``; the numbers of
  ``ffpa_attn_with_kvcache(q, kv_cache, kv_cache, ...)[..., :head_dim_v]``, from a kernel that fetches every latent row once (the K and the V^T fragments of a
  tile are read from one LDS image), packs the ``Hq / Hkv`` heads of a latent head into the rows of its tiles however many they are (128 heads x 1 token = two
  64-row workgroups per sequence), and stores no junk columns.

  ``kv_cache``: the page pool ``[num_pages, page_size, Hkv, D]`` with an int32 ``block_table [B, pages_per_seq]`` (``page_size`` a multiple of 64), or a contiguous
  ``[B, capacity, Hkv, D]`` without one.  The contiguous cache is served by the SAME paged kernel as a pool of one page per sequence, through an identity block
  table made on the device once per (B, device): it needs ``capacity % 64 == 0`` (``ValueError`` otherwise) and has no kernel of its own.  ``Hq % Hkv == 0``
  (``Hkv`` is 1 in the models named above; nothing assumes it).  ``cache_seqlens``: an int or an int32 ``[B]`` device tensor of keys per sequence.  ``causal`` is
  ``ffpa_attn_with_kvcache``'s: the last ``Sq`` keys are the queries' own.  A row that sees no key returns O = 0, LSE = -inf.

  ``softmax_scale`` is REQUIRED (``TypeError``): these models scale by ``1 / sqrt(qk_nope_head_dim + qk_rope_head_dim)`` = ``1 / sqrt(192)`` times their YaRN
  factor, which is not ``1 / sqrt(D)`` — a default would be silently wrong.

  Builds: ``(D, head_dim_v) = (576, 512)``, bf16 and fp16.  Both must be multiples of 64 with ``head_dim_v <= D`` (``ValueError``); any other pair raises
  ``NotImplementedError`` naming it.

  ``kv [B, Snew, Hkv, D]`` appends the step's latent rows in place at ``cache_seqlens[b] + i`` (dropped at or past the capacity; every element stored once:
  there is one cache) and attends over ``min(cache_seqlens + Snew, capacity)`` keys, as ``ffpa_attn_with_kvcache`` does with ``k`` / ``v``; ``cache_seqlens`` is
  not modified.  There are NO rotary parameters: these models rotate ``k_pe`` and ``q_pe`` before the concatenation, and their rotary columns sit at the END of
  the row — rotate before the call.

  Nothing is read back to the host: the call (append + attention + the split launch's merge) captures into one HIP graph, and a replay follows
  ``cache_seqlens``, ``block_table`` and ``kv`` written in place.  Inference only: a tensor that requires grad raises ``NotImplementedError``.  NOT served here,
  each raises ``NotImplementedError`` naming the keyword: ``window_size``, ``softcap``, ``tree_mask``, ``cu_seqlens_q`` (ragged batches are
  ``ffpa_attn_varlen_with_kvcache_mla``'s), shared-prefix cascades, ``rotary_cos`` / ``rotary_sin``, ALiBi, ``cache_batch_idx`` / ``cache_leftpad``.  FP8
  latents are a dtype error HERE: a ``torch.float8_e4m3fn`` cache is ``ffpa_attn_with_kvcache_mla_fp8``'s."""
  name = "ffpa_attn_with_kvcache_mla"
  if unsupported:
    raise NotImplementedError(f"{name} does not support: {', '.join(sorted(unsupported))} (no window, soft-cap, tree mask, cascade, rotary tables, ALiBi, batch "
                              "index or leftpad over the latent cache: rotate q_pe / k_pe before the call; a ragged batch — cu_seqlens_q — is "
                              "ffpa_attn_varlen_with_kvcache_mla's)")
  capacity, lens = _mla_check(name, q, kv_cache, head_dim_v, kv, cache_seqlens, block_table, softmax_scale, num_splits)
  return _mla_step(name, "mla", None, q, kv_cache, head_dim_v, kv, lens, block_table, capacity, softmax_scale, causal, num_splits, return_softmax_lse)


# ---- FP8 latent caches (OCP e4m3 codes, one per-tensor scale): ffpa_attn_with_kvcache_mla_fp8 / ffpa_attn_varlen_with_kvcache_mla_fp8
_E4M3_MAX = 448.0


def quantize_latent_rows(kv: torch.Tensor, kv_scale: float) -> torch.Tensor:
  """Latent rows ``kv`` (bf16 / fp16 / fp32, any shape) -> ``torch.float8_e4m3fn`` codes under the per-tensor dequantisation factor ``kv_scale`` (K = kv_scale x
  K8), by the definition the appends of the FP8 latent calls implement TO THE BIT::

      code = rne_e4m3(clamp(float32(x) * float32(1 / kv_scale), -448, +448))

  +-inf therefore saturates to +-448 and NaN stays NaN (torch's bare ``.to(torch.float8_e4m3fn)`` turns every overflow into NaN: the clamp is part of the
  definition).  Round to nearest even, subnormals kept (the smallest is 2^-9; +-2^-10 is a tie and goes to +-0).  Plain torch on any device: what a caller fills
  an FP8 pool with, and the reference the tests hold the append kernels to."""
  from .hip import check_kv_scale

  if not isinstance(kv, torch.Tensor) or not kv.is_floating_point():
    raise TypeError(f"quantize_latent_rows: kv must be a floating-point tensor, got {type(kv).__name__}")
  kv_scale = check_kv_scale(kv_scale, "quantize_latent_rows")
  inv = torch.tensor(1.0 / kv_scale, dtype=torch.float32, device=kv.device)
  v = kv.to(torch.float32) * inv
  v = torch.where(torch.isnan(v), v, v.clamp(-_E4M3_MAX, _E4M3_MAX))
  return v.to(torch.float8_e4m3fn)


# (tests/golden/mla_front_calls.json pins this text and the docstrings of the six calls it replays, byte for byte — the last clause here and the "FP8 pools in the
# sparse and the tree call" / "FP8 latents (a dtype error)" of those docstrings included, which ffpa_attn_with_kvcache_mla_sparse_fp8 and the two *_mla_tree_fp8 calls
# below have made stale: they stay as recorded until a change regenerates the golden.)
_MLA_FP8_UNSERVED = ("no window, soft-cap, tree mask, cascade, rotary tables, ALiBi, batch index or leftpad over the latent cache: rotate q_pe / k_pe before the "
                     "call; FP8 pools are not served by the sparse and the tree call")


def ffpa_attn_with_kvcache_mla_fp8(
  q: torch.Tensor,
  kv_cache: torch.Tensor,
  head_dim_v: int,
  *,
  kv_scale: float = 1.0,
  kv: torch.Tensor | None = None,
  cache_seqlens: "int | torch.Tensor",
  block_table: torch.Tensor | None = None,
  softmax_scale: float = _MLA_REQUIRED,
  causal: bool = False,
  num_splits: int = 0,
  return_softmax_lse: bool = False,
  **unsupported,
):
  """``ffpa_attn_with_kvcache_mla`` over an FP8 latent cache — the serving engines' ``kv_cache_dtype="fp8"`` for the MLA models: ``kv_cache`` is
  ``torch.float8_e4m3fn`` (OCP e4m3, the chip's FP8 format; ``float8_e4m3fnuz`` and the e5m2 formats raise ``TypeError``), the whole 576-wide row under ONE
  per-tensor scale, ``K = kv_scale * K8`` (the engines' ``k_scale``).  ``kv_scale`` is a host float, finite and positive (``ValueError``; a tensor raises
  ``TypeError``: a device scalar would need a read-back).  ``q``, ``kv`` and the output are bf16 or fp16.

  There is no FP8 arithmetic and no dequantised copy: every e4m3 value is exactly representable in bf16 and in fp16, so the kernel widens a tile on its way into
  LDS and runs the 16-bit latent kernel's MFMAs on it, and the scale never touches an element — the scores are ``(softmax_scale * kv_scale) * q.K8`` and
  ``O = kv_scale * sum p K8[:, :head_dim_v]``.  With a power-of-two ``kv_scale`` the call returns the bits of ``ffpa_attn_with_kvcache_mla(q,
  kv_cache.to(q.dtype), ..., softmax_scale=softmax_scale * kv_scale) * kv_scale``.

  ``kv [B, Snew, Hkv, D]`` (q's dtype) is QUANTISED by the append, one store per element, exactly as ``quantize_latent_rows(kv, kv_scale)`` — clamped to +-448,
  NaN kept.  Everything else is the latent call's: the page pool ``[num_pages, page_size, Hkv, D]`` with a ``block_table`` or a contiguous ``[B, capacity, Hkv,
  D]`` (strides multiples of 16 elements), the required ``softmax_scale``, the ``(576, 512)`` build, ``cache_seqlens``, ``causal``, ``num_splits``, one HIP graph for
  append + attention + merge, inference only, unsupported keywords refused by name.  Not served: per-token / per-block scales, FP8 ``q``, FP8 pools in the sparse
  and the tree call."""
  name = "ffpa_attn_with_kvcache_mla_fp8"
  if unsupported:
    raise NotImplementedError(f"{name} does not support: {', '.join(sorted(unsupported))} ({_MLA_FP8_UNSERVED}; a ragged batch — cu_seqlens_q — is "
                              "ffpa_attn_varlen_with_kvcache_mla_fp8's)")
  from . import hip  # (registers the ffpa_attn ops)

  kv_scale = hip.check_kv_scale(kv_scale, name)
  capacity, lens = _mla_check(name, q, kv_cache, head_dim_v, kv, cache_seqlens, block_table, softmax_scale, num_splits, fp8=True)
  return _mla_step(name, "fp8", kv_scale, q, kv_cache, head_dim_v, kv, lens, block_table, capacity, softmax_scale, causal, num_splits, return_softmax_lse)


def ffpa_attn_varlen_with_kvcache_mla_fp8(
  q: torch.Tensor,
  kv_cache: torch.Tensor,
  head_dim_v: int,
  cu_seqlens_q: torch.Tensor,
  max_seqlen_q: int,
  cache_seqlens: torch.Tensor,
  block_table: torch.Tensor | None = None,
  *,
  kv_scale: float = 1.0,
  kv: torch.Tensor | None = None,
  softmax_scale: float = _MLA_REQUIRED,
  causal: bool = False,
  num_splits: int = 0,
  return_softmax_lse: bool = False,
  **unsupported,
):
  """``ffpa_attn_varlen_with_kvcache_mla`` over an FP8 latent cache: the ragged step (``q [T, Hq, D]`` packed by ``cu_seqlens_q``) of
  ``ffpa_attn_with_kvcache_mla_fp8`` — ``kv_cache`` is ``torch.float8_e4m3fn`` under the per-tensor ``kv_scale`` (a host float), ``q``, ``kv [T, Hkv, D]`` and the
  output are bf16 or fp16, and ``kv`` is quantised by the ragged append as ``quantize_latent_rows(kv, kv_scale)``.  Shapes, the ``max_seqlen_q`` contract, the
  compact grid, the returned ``out [T, Hq, head_dim_v]`` / ``lse [Hq, T]`` and the one-graph step are ``ffpa_attn_varlen_with_kvcache_mla``'s; every sequence's rows
  are the bits of the uniform FP8 call on that sequence alone."""
  name = "ffpa_attn_varlen_with_kvcache_mla_fp8"
  if unsupported:
    raise NotImplementedError(f"{name} does not support: {', '.join(sorted(unsupported))} ({_MLA_FP8_UNSERVED})")
  from . import hip  # (registers the ffpa_attn ops)

  kv_scale = hip.check_kv_scale(kv_scale, name)
  capacity, lens = _mla_check(name, q, kv_cache, head_dim_v, kv, cache_seqlens, block_table, softmax_scale, num_splits, fp8=True, ragged=(cu_seqlens_q, max_seqlen_q))
  return _mla_step_varlen(name, "fp8", kv_scale, q, kv_cache, head_dim_v, cu_seqlens_q, max_seqlen_q, kv, lens, block_table, capacity, softmax_scale, causal, num_splits,
                          return_softmax_lse)


# ---- tree-mask attention over the MLA latent cache (the verification step of tree speculative decoding for the MLA models): ffpa_attn_with_kvcache_mla_tree
_MLA_TREE_UNSERVED = ("no causal flag — the mask says what a draft token sees —, no window, soft-cap, cascade, rotary tables, ALiBi, batch index or leftpad over "
                      "the latent cache: rotate q_pe / k_pe before the call")


def ffpa_attn_with_kvcache_mla_tree(
  q: torch.Tensor,
  kv_cache: torch.Tensor,
  head_dim_v: int,
  *,
  tree_mask: torch.Tensor,
  kv: torch.Tensor | None = None,
  cache_seqlens: "int | torch.Tensor",
  block_table: torch.Tensor | None = None,
  softmax_scale: float = _MLA_REQUIRED,
  num_splits: int = 0,
  return_softmax_lse: bool = False,
  **unsupported,
):
  """``ffpa_attn_with_kvcache_mla`` under a TREE MASK: the verification step of tree speculative decoding for the models whose cache is one latent pool (their MTP
  head driven as an EAGLE draft model with a tree of more than one branch).  The engine has appended — or appends here, with ``kv`` — the ``Sq`` draft nodes of
  every sequence to its latent cache and calls attention once: node i sees the whole prefix and, among the ``Sq`` draft rows, what ``tree_mask`` says.  ONE
  attention launch of the latent kernel's tree build: every latent row is fetched once, the ``Hq / Hkv`` heads x ``Sq`` tokens are the rows of
  ``ceil(Hq / Hkv * Sq / 64)`` tiles, and only the 32-key tiles that hold a draft row (at most three, and the tail) read the mask.  The launch and its plan are
  the causal latent call's; no call per root-to-leaf path, no two-cache kernel on an aliased pool.

  ``q [B, Sq, Hq, D]``, ``kv_cache``, ``head_dim_v``, ``kv``, ``cache_seqlens``, ``block_table``, the REQUIRED ``softmax_scale`` (``TypeError``), the ``(D,
  head_dim_v) = (576, 512)`` build, the contiguous cache (``capacity % 64 == 0``, one page per sequence), ``num_splits`` and the returns (``out [B, Sq, Hq,
  head_dim_v]``, fp32 ``lse [B, Hq, Sq]``) are ``ffpa_attn_with_kvcache_mla``'s.  ``tree_mask``: a ``torch.bool`` tensor on q's device, ``[W, W]`` (one tree for
  the batch) or ``[B, W, W]`` — or the int64 words ``[B | 1, W]`` ``pack_tree_mask`` makes of one —, ``Sq <= W <= 64``: the top-left ``Sq x Sq`` is read.  With
  ``L_b`` the rows attention runs over (``min(cache_seqlens[b] + Snew, capacity)`` with ``kv``, else ``cache_seqlens[b]`` clamped to the capacity), query token i
  of sequence b sees

  * row ``p`` for every ``p < L_b - Sq`` (the prefix), and
  * row ``L_b - Sq + j`` iff ``tree_mask[b, i, j]``; draft positions below 0 (``L_b < Sq``) do not exist.

  The mask is arbitrary: a False diagonal (one token per sequence included: ``[[False]]`` hides the token's own row) and "sees a later node" are legal;
  ``tril(ones)`` is ``ffpa_attn_with_kvcache_mla(causal=True)`` and all ones ``causal=False``, to the bit.  A row that sees nothing returns O = 0, LSE = -inf.
  Nothing is read back to the host: the call (append + attention + the split launch's merge) captures into one HIP graph, and a replay follows ``q``, ``kv``, the
  mask words (hand over packed words to write words), ``cache_seqlens`` and ``block_table`` written in place.  Inference only: a tensor that requires grad raises
  ``NotImplementedError``.  NOT served here, each raises ``NotImplementedError`` naming the keyword: ``causal`` (the mask says it), ``window_size``, ``softcap``,
  ``cu_seqlens_q`` (ragged batches are ``ffpa_attn_varlen_with_kvcache_mla_tree``'s), shared-prefix cascades, ``rotary_cos`` / ``rotary_sin``, ALiBi,
  ``cache_batch_idx`` / ``cache_leftpad``, masks over the prefix, more than 64 draft tokens and FP8 latents (a dtype error)."""
  name = "ffpa_attn_with_kvcache_mla_tree"
  if unsupported:
    raise NotImplementedError(f"{name} does not support: {', '.join(sorted(unsupported))} ({_MLA_TREE_UNSERVED}; a ragged batch — cu_seqlens_q — is "
                              "ffpa_attn_varlen_with_kvcache_mla_tree's)")
  capacity, lens = _mla_check(name, q, kv_cache, head_dim_v, kv, cache_seqlens, block_table, softmax_scale, num_splits)
  if isinstance(tree_mask, torch.Tensor) and tree_mask.requires_grad and torch.is_grad_enabled():
    raise NotImplementedError(f"{name} is inference only: tree_mask requires grad and there is no backward")
  return _mla_step(name, "tree", tree_mask, q, kv_cache, head_dim_v, kv, lens, block_table, capacity, softmax_scale, False, num_splits, return_softmax_lse)


def ffpa_attn_with_kvcache_mla_tree_fp8(
  q: torch.Tensor,
  kv_cache: torch.Tensor,
  head_dim_v: int,
  *,
  kv_scale: float = 1.0,
  tree_mask: torch.Tensor,
  kv: torch.Tensor | None = None,
  cache_seqlens: "int | torch.Tensor",
  block_table: torch.Tensor | None = None,
  softmax_scale: float = _MLA_REQUIRED,
  num_splits: int = 0,
  return_softmax_lse: bool = False,
  **unsupported,
):
  """``ffpa_attn_with_kvcache_mla_tree`` over an FP8 latent cache — the verification step of tree speculative decoding (MTP / EAGLE drafting) for an engine that
  keeps the latent cache as ``kv_cache_dtype="fp8"``: ``kv_cache`` is ``torch.float8_e4m3fn`` (OCP e4m3; ``float8_e4m3fnuz`` and the e5m2 formats raise
  ``TypeError``) under ONE per-tensor scale, ``K = kv_scale * K8``; ``kv_scale`` is a host float, finite and positive (``ValueError``; a tensor raises
  ``TypeError``).  ``q``, ``kv`` and the output are bf16 or fp16.  ``kv [B, Snew, Hkv, D]`` is QUANTISED by the FP8 latent call's append, exactly as
  ``quantize_latent_rows(kv, kv_scale)``.

  ``tree_mask``, what a draft token sees, the shapes, ``cache_seqlens``, ``block_table``, the contiguous cache, the required ``softmax_scale``, ``num_splits``, the
  returns and the one-graph step are ``ffpa_attn_with_kvcache_mla_tree``'s; the pool (strides multiples of 16 elements), the exact widening and the place of the
  scale are ``ffpa_attn_with_kvcache_mla_fp8``'s.  ``tril(ones)`` is ``ffpa_attn_with_kvcache_mla_fp8(causal=True)`` and all ones ``causal=False``, to the bit; with
  a power-of-two ``kv_scale`` the call returns the bits of ``ffpa_attn_with_kvcache_mla_tree(q, kv_cache.to(q.dtype), ..., softmax_scale=softmax_scale *
  kv_scale) * kv_scale``.  Not served: per-token / per-block scales, FP8 ``q``, a ``kv_scale`` on the device; every keyword the 16-bit call refuses."""
  name = "ffpa_attn_with_kvcache_mla_tree_fp8"
  if unsupported:
    raise NotImplementedError(f"{name} does not support: {', '.join(sorted(unsupported))} ({_MLA_TREE_UNSERVED}; a ragged batch — cu_seqlens_q — is "
                              "ffpa_attn_varlen_with_kvcache_mla_tree_fp8's)")
  from . import hip  # (registers the ffpa_attn ops)

  kv_scale = hip.check_kv_scale(kv_scale, name)
  capacity, lens = _mla_check(name, q, kv_cache, head_dim_v, kv, cache_seqlens, block_table, softmax_scale, num_splits, fp8=True)
  if isinstance(tree_mask, torch.Tensor) and tree_mask.requires_grad and torch.is_grad_enabled():
    raise NotImplementedError(f"{name} is inference only: tree_mask requires grad and there is no backward")
  return _mla_step(name, "tree_fp8", (tree_mask, kv_scale), q, kv_cache, head_dim_v, kv, lens, block_table, capacity, softmax_scale, False, num_splits,
                   return_softmax_lse)


# ---- ragged query batches (continuous batching, chunked prefill): ffpa_attn_varlen_with_kvcache
# ----------------------------------------------------------------------------- sparse (top-k indexed) attention over the latent cache
def compact_topk_indices(indices: torch.Tensor) -> "tuple[torch.Tensor, torch.Tensor]":
  """``indices [..., topk]`` with ``-1`` (any negative entry) for "no key" anywhere in a row -> ``(indices with every row's entries >= 0 moved to the front in
  their order, int32 counts [...])``: the form ``ffpa_attn_with_kvcache_mla_sparse`` takes (its kernel serves no holes inside a row).  A stable sort on
  validity and a sum: plain torch, no host read — it captures into a graph.  What follows a row's valid entries are its invalid ones, as they were."""
  if not isinstance(indices, torch.Tensor) or indices.dtype not in (torch.int32, torch.int64) or indices.dim() < 1:
    raise ValueError("compact_topk_indices: indices must be an int32 / int64 tensor [..., topk]")
  valid = indices >= 0
  order = torch.sort((~valid).to(torch.int8), dim=-1, stable=True).indices
  return torch.gather(indices, -1, order), valid.sum(dim=-1, dtype=torch.int32)


def slots_from_block_table(positions: torch.Tensor, block_table: torch.Tensor, page_size: int) -> torch.Tensor:
  """Logical key positions ``[T, topk]`` of sequences -> int32 slots of a page pool: position p of the sequence whose row of page ids is ``block_table[t]``
  (``[T, pages_per_seq]``: one row per token — index the sequences' table by the tokens' sequence ids first) lives in slot
  ``block_table[t, p // page_size] * page_size + p % page_size``.  ``positions < 0`` stay -1.  Plain torch, no host read."""
  if positions.dim() != 2 or block_table.dim() != 2 or block_table.size(0) != positions.size(0):
    raise ValueError("slots_from_block_table: positions must be [T, topk] and block_table [T, pages_per_seq]")
  if isinstance(page_size, bool) or not isinstance(page_size, int) or page_size <= 0:
    raise ValueError(f"slots_from_block_table: page_size must be a positive int, got {page_size!r}")
  pos = positions.to(torch.int64)
  live = pos >= 0
  safe = torch.where(live, pos, torch.zeros_like(pos))
  page = torch.gather(block_table.to(torch.int64), 1, (safe // page_size).clamp_(max=max(block_table.size(1) - 1, 0)))
  return torch.where(live, page * page_size + safe % page_size, torch.full_like(pos, -1)).to(torch.int32)


def _mla_sparse_select_check(name, rows, what, dtype, topk, cache_seqlens, block_table, page_size, cu_seqlens_q) -> int:
  """The argument checks of ``ffpa_mla_sparse_topk_slots`` / ``ffpa_mla_sparse_slots`` under their own ``name`` (``rows``: the scores or the positions, ``what``
  its name) -> ``page_size`` as the op takes it (1 without a table).  ``TypeError`` for types and dtypes, ``NotImplementedError`` for a tensor that requires grad,
  ``ValueError`` for shapes, devices and strides; nothing is read from the device."""
  tensors = ((what, rows), ("cache_seqlens", cache_seqlens)) + ((("block_table", block_table),) if block_table is not None else ()) + \
            ((("cu_seqlens_q", cu_seqlens_q),) if cu_seqlens_q is not None else ())
  for nm, t in tensors:
    if not isinstance(t, torch.Tensor):
      raise TypeError(f"{name}: {nm} must be a tensor, got {type(t).__name__}")
    if t.requires_grad and torch.is_grad_enabled():
      raise NotImplementedError(f"{name} is inference only: {nm} requires grad and there is no backward")
  if rows.dtype != dtype:
    raise TypeError(f"{name}: {what} must be {dtype}, got {rows.dtype}" + (" (bf16 / fp16 scores are not served: hand over .float())" if rows.is_floating_point() else ""))
  for nm, t in tensors[1:]:
    if t.dtype != torch.int32:
      raise TypeError(f"{name}: {nm} must be an int32 tensor, got {t.dtype}")
  if isinstance(topk, bool) or not isinstance(topk, int):
    raise TypeError(f"{name}: topk must be an int, got {topk!r}")
  if block_table is not None and (isinstance(page_size, bool) or not isinstance(page_size, int)):
    raise TypeError(f"{name}: with a block_table page_size must be an int, got {page_size!r}")
  if rows.dim() != 2 or rows.size(1) < 1:
    raise ValueError(f"{name}: {what} must be [T, {'N' if what == 'scores' else 'topk'}] with at least one column, got {tuple(rows.shape)}")
  T, N = rows.shape
  if topk < 1 or topk > N:
    raise ValueError(f"{name}: topk must lie in [1, N={N}], got {topk}")
  if N > 1 << 30:
    raise ValueError(f"{name}: rows of more than 2^30 columns are not served, got {N}")
  if rows.stride(1) != 1:
    raise ValueError(f"{name}: {what} must have a contiguous last dimension (the row stride is free)")
  if cache_seqlens.dim() != 1 or cache_seqlens.numel() < 1:
    raise ValueError(f"{name}: cache_seqlens must be an int32 tensor [B] with B >= 1, got {tuple(cache_seqlens.shape)}")
  B = cache_seqlens.numel()
  if cu_seqlens_q is not None and (cu_seqlens_q.dim() != 1 or cu_seqlens_q.numel() != B + 1):
    raise ValueError(f"{name}: cu_seqlens_q must be an int32 tensor [B + 1 = {B + 1}], got {tuple(cu_seqlens_q.shape)}")
  if cu_seqlens_q is None and T % B != 0:
    raise ValueError(f"{name}: without cu_seqlens_q the T={T} rows are [B, Sq] flattened: T must be a multiple of B={B}")
  if block_table is not None:
    if page_size < 1:
      raise ValueError(f"{name}: page_size must be a positive int, got {page_size!r}")
    if block_table.dim() != 2 or block_table.size(0) != B or block_table.size(1) < 1:
      raise ValueError(f"{name}: block_table must be [B={B}, pages_per_seq >= 1] — one row per SEQUENCE —, got {tuple(block_table.shape)}")
    if block_table.stride(1) != 1:
      raise ValueError(f"{name}: block_table must have a contiguous last dimension (the row stride is free)")
  for nm, t in tensors[1:]:
    if t.device != rows.device:
      raise ValueError(f"{name}: {nm} must be on {what}'s device, got {t.device} and {rows.device}")
  return page_size if block_table is not None else 1


def ffpa_mla_sparse_topk_slots(
  scores: torch.Tensor,
  topk: int,
  cache_seqlens: torch.Tensor,
  block_table: "torch.Tensor | None" = None,
  page_size: "int | None" = None,
  *,
  cu_seqlens_q: "torch.Tensor | None" = None,
  causal: bool = True,
) -> "tuple[torch.Tensor, torch.Tensor]":
  """From an indexer's scores to the inputs of the sparse latent calls, in ONE launch: ``scores`` — float32 ``[T, N]`` on the GPU, unit stride in the last
  dimension, free row stride; column ``p`` is the score of logical key position ``p`` of the token's sequence — -> ``(indices int32 [T, topk], topk_lens int32
  [T])``, exactly the pair ``ffpa_attn_with_kvcache_mla_sparse`` / ``_sparse_fp8`` / ``_sparse_ds`` take, on the device (SGLang's ``fast_topk_transform_fused``,
  vLLM's ``top_k_per_row`` + ``convert_req_index_to_global_index``).  It replaces ``torch.topk``, a per-token table gather, ``slots_from_block_table`` and
  ``compact_topk_indices`` — about a dozen launches, two of them sorts — in front of every layer's attention.

  Token -> sequence: ``cu_seqlens_q`` (int32 ``[B + 1]``) packs the rows as the ragged latent calls do — rows at and past ``cu_seqlens_q[B]`` are padding: count
  0, a row of -1 —; without it ``T % B == 0``, ``Sq = T // B`` and row ``t`` is token ``t % Sq`` of sequence ``t // Sq``.  ``cache_seqlens``: int32 ``[B]``, the
  lengths WITH the step's rows in the cache (the sparse call has no ``kv=``).  Token ``i`` of a sequence of ``S`` query tokens and length ``L`` sees the columns
  ``[0, n)``, ``n = clamp(L - (S - 1 - i), 0, N)`` under ``causal`` (the bottom-right alignment of every ragged call here), ``clamp(L, 0, N)`` otherwise; columns
  at and past ``n`` are never selected, whatever they hold.

  The selection is a pure function of its inputs: ``n <= topk`` selects all of ``0 ... n - 1``; otherwise the ``topk`` largest of the first ``n`` scores in the
  order of ``torch.sort(descending=True, stable=True)`` — NaN counts as the largest value, -0.0 equals +0.0, among equal scores the lower position wins.  The
  selected positions are written in ASCENDING position order (the pages are walked front to back; with ``n <= topk`` the row lists the sequence's slots in order,
  the case in which the sparse call returns the dense latent call's bits), entries at and past the count are -1, ``topk_lens[t] = min(n, topk)``.  ``topk``: a
  host int in ``[1, N]``, no power-of-two requirement.

  Translation: position ``p`` of sequence ``b`` becomes ``block_table[b, min(p // page_size, W - 1)] * page_size + p % page_size`` — ``block_table`` int32
  ``[B, W]``, one row per SEQUENCE (not per token, as ``slots_from_block_table`` wants it), free row stride; ``page_size`` any positive int.  ``block_table=None``
  writes the positions themselves.  Page ids are not validated: the sparse call clamps slots into the pool.

  One HIP kernel, a workgroup per row (a long row is not split over workgroups); nothing is read back to the host, so the call captures into a HIP graph in front
  of the sparse call and a replay follows ``scores``, ``cache_seqlens``, ``cu_seqlens_q`` and ``block_table`` written in place.  ``T == 0`` returns empty tensors
  and launches nothing.  Not served: bf16 scores (``TypeError``), per-head index rows."""
  name = "ffpa_mla_sparse_topk_slots"
  page_size = _mla_sparse_select_check(name, scores, "scores", torch.float32, topk, cache_seqlens, block_table, page_size, cu_seqlens_q)
  from . import hip  # noqa: F401  (registers the ffpa_attn ops)

  if scores.size(0) == 0:
    return scores.new_empty((0, topk), dtype=torch.int32), scores.new_empty((0,), dtype=torch.int32)
  return torch.ops.ffpa_attn._mla_sparse_topk_slots_hip(scores, topk, cache_seqlens, block_table, page_size, cu_seqlens_q, bool(causal))


def ffpa_mla_sparse_slots(
  positions: torch.Tensor,
  cache_seqlens: torch.Tensor,
  block_table: "torch.Tensor | None" = None,
  page_size: "int | None" = None,
  *,
  cu_seqlens_q: "torch.Tensor | None" = None,
) -> "tuple[torch.Tensor, torch.Tensor]":
  """``ffpa_mla_sparse_topk_slots``'s last phase for an engine that keeps its own top-k: ``positions`` — int32 ``[T, topk]`` on the GPU, logical key positions
  with negative entries ("no key") anywhere in a row — -> ``(indices int32 [T, topk], topk_lens int32 [T])``: the entries ``>= 0`` keep their order and move to the
  front, translated through the sequence's row of ``block_table`` (as there; ``None``: as they are), the count is their number, the tail is -1.  On the front
  entries and the counts that is ``compact_topk_indices(slots_from_block_table(positions, block_table[sequence of each token], page_size))`` in ONE launch of the
  same kernel, with the table indexed per sequence on the device.  Token -> sequence is ``ffpa_mla_sparse_topk_slots``'s rule (``cu_seqlens_q``, or ``T % B == 0``;
  padding rows: count 0, a row of -1); ``cache_seqlens`` (int32 ``[B]``) names the sequences — no length is applied, the caller's top-k has chosen visible keys.
  Nothing is read back to the host; ``T == 0`` returns empty tensors and launches nothing."""
  name = "ffpa_mla_sparse_slots"
  topk = positions.size(1) if isinstance(positions, torch.Tensor) and positions.dim() == 2 and positions.size(1) >= 1 else 1
  page_size = _mla_sparse_select_check(name, positions, "positions", torch.int32, topk, cache_seqlens, block_table, page_size, cu_seqlens_q)
  from . import hip  # noqa: F401  (registers the ffpa_attn ops)

  if positions.size(0) == 0:
    return positions.new_empty((0, topk)), positions.new_empty((0,))
  return torch.ops.ffpa_attn._mla_sparse_slots_hip(positions, cache_seqlens, block_table, page_size, cu_seqlens_q)


def _mla_sparse_check(name, q, kv_cache, head_dim_v, indices, topk_lens, softmax_scale, num_splits, fp8=False, ds=False):
  """The argument checks of the sparse latent calls under their own ``name``, every rule written once and in the order ``ffpa_attn_with_kvcache_mla_sparse`` has
  always made them -> ``(T, Hq)``.  ``fp8``: the pool is ``torch.float8_e4m3fn`` (``ffpa_attn_with_kvcache_mla_sparse_fp8``) — the dtype rule is the FP8 latent
  calls', and ``mla_sparse_pool`` holds the pool to the FP8 stride rule and counts its span in its own bytes.  ``ds``: the pool is ``torch.uint8`` rows of 656
  bytes (``ffpa_attn_with_kvcache_mla_sparse_ds``) under a bf16 ``q`` — its last dimension is the row's bytes, and ``mla_sparse_ds_pool`` holds its geometry."""
  if softmax_scale is _MLA_REQUIRED or softmax_scale is None:
    raise TypeError(f"{name}: softmax_scale is required — an MLA model scales by 1 / sqrt(qk_nope_head_dim + qk_rope_head_dim) (x its YaRN factor), which is not "
                    "1 / sqrt(D) of the 576-wide absorbed head: there is no right default")
  if isinstance(softmax_scale, bool) or not isinstance(softmax_scale, (int, float)):
    raise TypeError(f"{name}: softmax_scale must be a real number, got {softmax_scale!r}")
  for nm, t in (("q", q), ("kv_cache", kv_cache), ("indices", indices)) + ((("topk_lens", topk_lens),) if topk_lens is not None else ()):
    if not isinstance(t, torch.Tensor):
      raise TypeError(f"{name}: {nm} must be a tensor, got {type(t).__name__}")
    if t.requires_grad and torch.is_grad_enabled():
      raise NotImplementedError(f"{name} is inference only: {nm} requires grad and there is no backward")
  if ds:
    if q.dtype != torch.bfloat16 or kv_cache.dtype != torch.uint8:
      raise TypeError(f"{name} only supports bf16 q over a torch.uint8 kv_cache of {_DS_ROW_BYTES}-byte rows — the rotary columns of a row are bf16 and are read "
                      f"as they are; fp16 q is not served —, got {q.dtype}, {kv_cache.dtype}")
  elif fp8:
    if q.dtype not in _DTYPES or kv_cache.dtype != torch.float8_e4m3fn:
      raise TypeError(f"{name} only supports fp16/bf16 q over a torch.float8_e4m3fn kv_cache — OCP e4m3 is the chip's FP8 format; float8_e4m3fnuz and the e5m2 "
                      f"formats are not served —, got {q.dtype}, {kv_cache.dtype}")
  elif q.dtype not in _DTYPES or kv_cache.dtype != q.dtype:
    raise TypeError(f"{name} only supports fp16/bf16 q/kv_cache of one dtype, got {q.dtype}, {kv_cache.dtype}")
  if q.dim() != 3 or kv_cache.dim() not in (3, 4):
    raise ValueError(f"{name}: q must be [T, Hq, D] (flatten a [B, Sq, Hq, D] step) and kv_cache [num_rows, Hkv, D] or [num_pages, page_size, Hkv, D]")
  T, Hq, D = q.shape
  Hkv = kv_cache.size(-2)
  if ds and kv_cache.size(-1) != _DS_ROW_BYTES:
    raise ValueError(f"{name}: the last dimension of the cache ({kv_cache.size(-1)}) must be the {_DS_ROW_BYTES} bytes of a row")
  if not ds and kv_cache.size(-1) != D:
    raise ValueError(f"{name}: head dim of the cache ({kv_cache.size(-1)}) differs from q's ({D})")
  if isinstance(head_dim_v, bool) or not isinstance(head_dim_v, int):
    raise TypeError(f"{name}: head_dim_v must be an int, got {head_dim_v!r}")
  if D % 64 != 0 or head_dim_v <= 0 or head_dim_v % 64 != 0 or head_dim_v > D:
    raise ValueError(f"{name}: (D, head_dim_v) = ({D}, {head_dim_v}): both must be multiples of 64 with 0 < head_dim_v <= D")
  from .hip import MLA_BUILDS, mla_sparse_ds_pool, mla_sparse_pool

  if (D, head_dim_v) not in MLA_BUILDS:
    raise NotImplementedError(f"{name}: (D, head_dim_v) = ({D}, {head_dim_v}) is not built (built: {', '.join(map(str, MLA_BUILDS))})")
  if Hkv == 0 or Hq % Hkv != 0:
    raise ValueError(f"{name}: query num_heads ({Hq}) must be a multiple of the latent num_heads ({Hkv})")
  if isinstance(num_splits, bool) or not isinstance(num_splits, int) or num_splits < 0:
    raise ValueError(f"{name}: num_splits must be a non-negative int, got {num_splits!r}")
  if kv_cache.device != q.device:
    raise ValueError(f"{name}: q / kv_cache must be on one device, got {q.device}, {kv_cache.device}")
  if kv_cache.stride(-1) != 1:
    raise ValueError(f"{name}: kv_cache must have a contiguous last dimension")
  if indices.dim() == 3:
    raise NotImplementedError(f"{name}: per-head index rows ([T, Hkv, topk]) are not served: all latent heads of a token share one row [T, topk]")
  if indices.dtype != torch.int32 or indices.dim() != 2 or indices.size(0) != T:
    raise ValueError(f"{name}: indices must be an int32 tensor [T={T}, topk], got {indices.dtype} {tuple(indices.shape)}")
  if indices.size(1) < 1:
    raise ValueError(f"{name}: indices needs at least one entry per token (topk >= 1)")
  if indices.stride(1) != 1:
    raise ValueError(f"{name}: indices must have a contiguous last dimension")
  if indices.device != q.device:
    raise ValueError(f"{name}: indices must be on q's device, got {indices.device} and {q.device}")
  if topk_lens is not None and (topk_lens.dtype != torch.int32 or topk_lens.dim() != 1 or topk_lens.numel() != T or topk_lens.device != q.device):
    raise ValueError(f"{name}: topk_lens must be an int32 tensor [T={T}] on q's device")
  if kv_cache.numel() == 0:
    raise ValueError(f"{name}: kv_cache must be a non-empty pool")
  (mla_sparse_ds_pool if ds else mla_sparse_pool)(kv_cache, name)  # (evenly spaced pages, the span the kernel's offsets reach, a byte pool's strides: ValueError)
  return T, Hq


def ffpa_attn_with_kvcache_mla_sparse(
  q: torch.Tensor,
  kv_cache: torch.Tensor,
  head_dim_v: int,
  indices: torch.Tensor,
  *,
  topk_lens: "torch.Tensor | None" = None,
  softmax_scale: float = _MLA_REQUIRED,
  num_splits: int = 0,
  return_softmax_lse: bool = False,
  **unsupported,
):
  """SPARSE attention over an MLA latent cache — DeepSeek-V3.2's "DeepSeek Sparse Attention" in its absorbed decode form (FlashMLA's sparse decode call): an
  indexer has picked ``topk`` latent rows per query token, shared by all heads of the token, and ``q [T, Hq, D]`` — the step's query tokens, flat (a
  ``[B, Sq, Hq, D]`` caller reshapes: every token brings its own keys) — attends to those rows only.  Returns ``out [T, Hq, head_dim_v]`` and, with
  ``return_softmax_lse``, the fp32 ``lse [Hq, T]`` (the ragged latent call's layout).  The rows are read where they lie: the kernel is a build of
  ``ffpa_attn_with_kvcache_mla``'s whose LDS-DMA pieces take their row from the index list — no gathered copy, no second launch.

  ``kv_cache``: the flat latent pool ``[num_rows, Hkv, D]``, or a page pool ``[num_pages, page_size, Hkv, D]`` of ANY positive ``page_size`` whose pages are
  evenly spaced (``stride(0) == page_size * stride(1)``, else ``ValueError``): slot r is row ``r % page_size`` of page ``r // page_size``.  Row and head strides
  are free, the last dimension has unit stride; keys are a row's ``D`` columns, values its first ``head_dim_v``.  ``(D, head_dim_v)`` = (576, 512), bf16 / fp16,
  ``Hq % Hkv == 0``.  The rows of a latent head may span at most 2^31 bytes — ``(num_rows - 1) * row stride + one row``, about 1.86 M dense 576-wide rows:
  the kernel's offsets are 32-bit with one bit spent on "no row" — a larger pool raises ``ValueError`` before any launch (hand over a view of the part the
  step's slots lie in).

  ``indices``: int32 ``[T, topk]`` on the device (unit stride in the last dimension, ``topk >= 1``), entry ``[t, j]`` a slot of the pool; duplicates are legal
  and count twice, as in a gather.  A 3-D ``[T, Hkv, topk]`` (per-head rows) raises ``NotImplementedError``.  ``topk_lens``: int32 ``[T]`` on the device, or
  ``None`` = every row holds ``topk`` valid entries; token t attends to ``indices[t, :clamp(topk_lens[t], 0, topk)]``.  Entries at and past the count are NEVER
  turned into an address, whatever they hold (engines pad with -1).  Entries in front of it must lie in ``[0, num_rows)``; one that does not is clamped into the
  pool — memory-safe, the token's result unspecified.  -1 holes INSIDE a row are not served: ``compact_topk_indices`` moves a row's valid entries to the front
  and counts them (plain torch, capturable); ``slots_from_block_table`` turns logical key positions into slots.  A token with count 0 returns O = 0 and
  LSE = -inf; ``T == 0`` returns empty tensors and launches nothing.

  ``softmax_scale`` is REQUIRED (``TypeError``), as in the two latent calls.  There is no ``causal`` (the indexer has chosen visible keys) and no ``kv=`` (the
  step's rows are appended by the latent calls or by the engine).  Nothing is read back to the host: the call — with the merge of a split launch — captures
  into one HIP graph, and a replay follows ``q``, ``indices``, ``topk_lens`` and the pool written in place.  Inference only: a tensor that requires grad raises
  ``NotImplementedError``.  NOT served, each raises ``NotImplementedError`` naming the keyword: ``causal``, ``kv``, ``window_size``, ``softcap``, ``tree_mask``,
  rotary tables, ALiBi, ``cache_batch_idx`` / ``cache_leftpad``.  FP8 latents are a dtype error HERE: a ``torch.float8_e4m3fn`` pool is
  ``ffpa_attn_with_kvcache_mla_sparse_fp8``'s."""
  name = "ffpa_attn_with_kvcache_mla_sparse"
  if unsupported:
    raise NotImplementedError(f"{name} does not support: {', '.join(sorted(unsupported))} (no causal flag — the indexer has chosen visible keys —, no kv= append, "
                              "no window, soft-cap, tree mask, rotary tables, ALiBi, batch index or leftpad over the sparse latent call)")
  T, Hq = _mla_sparse_check(name, q, kv_cache, head_dim_v, indices, topk_lens, softmax_scale, num_splits)
  from . import hip  # noqa: F401  (registers the ffpa_attn ops)

  if T == 0:
    out = q.new_empty((0, Hq, head_dim_v))
    return (out, q.new_empty((Hq, 0), dtype=torch.float32)) if return_softmax_lse else out
  out, lse = torch.ops.ffpa_attn._mla_sparse_fwd_hip(q, kv_cache, head_dim_v, indices, topk_lens, float(softmax_scale), num_splits)
  return (out, lse) if return_softmax_lse else out


def ffpa_attn_with_kvcache_mla_sparse_fp8(
  q: torch.Tensor,
  kv_cache: torch.Tensor,
  head_dim_v: int,
  indices: torch.Tensor,
  *,
  kv_scale: float = 1.0,
  topk_lens: "torch.Tensor | None" = None,
  softmax_scale: float = _MLA_REQUIRED,
  num_splits: int = 0,
  return_softmax_lse: bool = False,
  **unsupported,
):
  """``ffpa_attn_with_kvcache_mla_sparse`` over an FP8 latent pool — DeepSeek-V3.2's top-k attention as an engine with ``kv_cache_dtype="fp8"`` issues it:
  ``kv_cache`` is ``torch.float8_e4m3fn`` (OCP e4m3; ``float8_e4m3fnuz`` and the e5m2 formats raise ``TypeError``), the whole 576-wide row under ONE per-tensor
  scale, ``K = kv_scale * K8``.  ``kv_scale`` is a host float, finite and positive (``ValueError``; a tensor raises ``TypeError``).  ``q`` and the output are bf16
  or fp16.  The rows are read where they lie, as codes: the kernel is the sparse kernel's build whose pieces are 8-byte register loads at the gathered offsets,
  widened exactly on their way into LDS — no dequantised scratch pool, no gathered copy.  The scale never touches an element: the scores are ``(softmax_scale *
  kv_scale) * q.K8`` and ``O = kv_scale * sum p K8[:, :head_dim_v]``; with a power-of-two ``kv_scale`` the call returns the bits of
  ``ffpa_attn_with_kvcache_mla_sparse(q, kv_cache.to(q.dtype), ..., softmax_scale=softmax_scale * kv_scale) * kv_scale``.

  The pool's two forms, ``indices`` / ``topk_lens`` and their safety rules (entries at and past the count are never turned into an address, entries in front of it
  are clamped into the pool), the required ``softmax_scale``, the ``(576, 512)`` build, ``num_splits``, the returns (``out [T, Hq, head_dim_v]``, fp32 ``lse [Hq,
  T]``) and the one-graph call are ``ffpa_attn_with_kvcache_mla_sparse``'s.  Two rules are the FP8 pool's own (``ValueError`` before any launch): the row and
  head strides must be multiples of 16 elements, and the rows of a latent head may span at most 2^31 BYTES — for a pool of one byte per element that is twice as
  many rows, about 3.7 M dense 576-wide rows.  No ``kv=``: the step's rows are appended by the FP8 latent calls or by the engine
  (``quantize_latent_rows``).  Per-block scales inside the row — the 656-byte row layout of DeepSeek-V3.2 — are ``ffpa_attn_with_kvcache_mla_sparse_ds``'s.
  Not served: FP8 ``q``, a ``kv_scale`` on the device."""
  name = "ffpa_attn_with_kvcache_mla_sparse_fp8"
  if unsupported:
    raise NotImplementedError(f"{name} does not support: {', '.join(sorted(unsupported))} (no causal flag — the indexer has chosen visible keys —, no kv= append, "
                              "no window, soft-cap, tree mask, rotary tables, ALiBi, batch index or leftpad over the sparse latent call)")
  from . import hip  # (registers the ffpa_attn ops)

  kv_scale = hip.check_kv_scale(kv_scale, name)
  T, Hq = _mla_sparse_check(name, q, kv_cache, head_dim_v, indices, topk_lens, softmax_scale, num_splits, fp8=True)
  if T == 0:
    out = q.new_empty((0, Hq, head_dim_v))
    return (out, q.new_empty((Hq, 0), dtype=torch.float32)) if return_softmax_lse else out
  out, lse = torch.ops.ffpa_attn._mla_sparse_fp8_fwd_hip(q, kv_cache, head_dim_v, kv_scale, indices, topk_lens, float(softmax_scale), num_splits)
  return (out, lse) if return_softmax_lse else out


# ---- the 656-byte FP8 latent rows of DeepSeek-V3.2 (vLLM's "fp8_ds_mla", the FP8 KV layout of FlashMLA's sparse decode): the format, the store, the sparse call
_DS_NOPE, _DS_TILE, _DS_ROPE, _DS_ROW_BYTES = 512, 128, 64, 656
_DS_SCALE_FLOOR = 2.0 ** -100


def pack_latent_rows_ds(kv: torch.Tensor) -> torch.Tensor:
  """Latent rows ``kv [..., 576]`` (bf16 / fp16 / fp32) -> ``torch.uint8 [..., 656]``, the row format in which the engines keep DeepSeek-V3.2's latent cache::

      bytes   0 ... 511   the 512 latent ("NoPE") columns as OCP e4m3 codes
      bytes 512 ... 527   four little-endian float32 scales, one per 128 columns
      bytes 528 ... 655   the 64 rotary columns as bf16, not quantised

  For each 128-column tile ``x`` of the first 512 columns: ``a = amax(|float32(x)|)`` with non-finite elements counted as 0, ``s = max(a / 448, 2^-100)`` in
  float32, ``code = rne_e4m3(clamp(float32(x) / s, -448, +448))`` — IEEE divisions; NaN stays NaN (the code keeps x's sign) and +-inf saturates, the clamp and
  NaN rule of ``quantize_latent_rows``.  Plain torch on any device: THE DEFINITION ``store_latent_rows_ds``'s kernel implements to the byte."""
  if not isinstance(kv, torch.Tensor) or kv.dtype not in (torch.bfloat16, torch.float16, torch.float32):
    raise TypeError(f"pack_latent_rows_ds: kv must be a bf16 / fp16 / fp32 tensor, got {kv.dtype if isinstance(kv, torch.Tensor) else type(kv).__name__}")
  if kv.dim() < 1 or kv.size(-1) != _DS_NOPE + _DS_ROPE:
    raise ValueError(f"pack_latent_rows_ds: kv must be [..., {_DS_NOPE + _DS_ROPE}], got {tuple(kv.shape)}")
  x = kv[..., :_DS_NOPE].to(torch.float32).unflatten(-1, (_DS_NOPE // _DS_TILE, _DS_TILE))
  a = torch.where(torch.isfinite(x), x.abs(), torch.zeros_like(x)).amax(dim=-1, keepdim=True)
  s = (a / torch.full_like(a, _E4M3_MAX)).clamp_min(_DS_SCALE_FLOOR)  # (tensor / tensor: by a Python scalar torch multiplies by 1 / 448 on the GPU — not this division)
  v = x / s
  codes = torch.where(torch.isnan(x), x, v.clamp(-_E4M3_MAX, _E4M3_MAX)).to(torch.float8_e4m3fn).flatten(-2)  # (x's own NaN: the sign of NaN / s is the platform's)
  rope = kv[..., _DS_NOPE:].to(torch.bfloat16).contiguous()
  return torch.cat([codes.view(torch.uint8), s.squeeze(-1).contiguous().view(torch.uint8), rope.view(torch.uint8)], dim=-1)


def unpack_latent_rows_ds(rows: torch.Tensor) -> torch.Tensor:
  """``torch.uint8 [..., 656]`` rows of ``pack_latent_rows_ds``'s format -> bf16 ``[..., 576]``: latent column ``c`` is ``bf16_rne(float32(code[c]) *
  scale[c // 128])`` — ONE float32 multiply, then ONE round-to-nearest-even to bf16 —, the rotary bytes are reinterpreted, not converted.  THE DEFINITION of what
  ``ffpa_attn_with_kvcache_mla_sparse_ds`` computes on.  A scale outside ``[2^-100, 2^100]`` or not finite, in a pool somebody else packed, gives unspecified
  values for its 128 columns and nothing else: no address depends on a scale.  The last dimension must have unit stride; rows may be strided."""
  if not isinstance(rows, torch.Tensor) or rows.dtype != torch.uint8:
    raise TypeError(f"unpack_latent_rows_ds: rows must be a torch.uint8 tensor, got {rows.dtype if isinstance(rows, torch.Tensor) else type(rows).__name__}")
  if rows.dim() < 1 or rows.size(-1) != _DS_ROW_BYTES:
    raise ValueError(f"unpack_latent_rows_ds: rows must be [..., {_DS_ROW_BYTES}], got {tuple(rows.shape)}")
  codes = rows[..., :_DS_NOPE].contiguous().view(torch.float8_e4m3fn).to(torch.float32).unflatten(-1, (_DS_NOPE // _DS_TILE, _DS_TILE))
  s = rows[..., _DS_NOPE:_DS_NOPE + 16].contiguous().view(torch.float32).unsqueeze(-1)
  rope = rows[..., _DS_NOPE + 16:].contiguous().view(torch.bfloat16)
  return torch.cat([(codes * s).to(torch.bfloat16).flatten(-2), rope], dim=-1)


def store_latent_rows_ds(kv_cache: torch.Tensor, kv: torch.Tensor, slots: torch.Tensor) -> None:
  """Write the step's new latent rows into a pool of 656-byte rows BY SLOT, as the engines write this cache (``slot_mapping``): row ``t`` of the bf16 ``kv [T, Hkv,
  576]`` goes, packed as ``pack_latent_rows_ds(kv[t])`` to the byte, to slot ``slots[t]`` of ``kv_cache`` — ``torch.uint8``, ``[num_rows, Hkv, 656]`` or a page
  pool ``[num_pages, page_size, Hkv, 656]`` with evenly spaced pages, written in place.  ``slots``: int32 ``[T]`` on the device; a slot ``< 0`` (the engines'
  padding) or ``>= num_rows`` writes nothing, and two tokens with one slot are the caller's error (one of them wins).  ONE kernel, nothing read back to the host:
  it captures into a HIP graph in front of ``ffpa_attn_with_kvcache_mla_sparse_ds``.  ``kv`` may be strided in its token and head dimensions."""
  name = "store_latent_rows_ds"
  for nm, t in (("kv_cache", kv_cache), ("kv", kv), ("slots", slots)):
    if not isinstance(t, torch.Tensor):
      raise TypeError(f"{name}: {nm} must be a tensor, got {type(t).__name__}")
  if kv.dtype != torch.bfloat16 or kv_cache.dtype != torch.uint8:
    raise TypeError(f"{name} only supports bf16 kv over a torch.uint8 kv_cache of {_DS_ROW_BYTES}-byte rows, got {kv.dtype}, {kv_cache.dtype}")
  if kv.dim() != 3 or kv.size(-1) != _DS_NOPE + _DS_ROPE or kv_cache.dim() not in (3, 4) or kv_cache.size(-1) != _DS_ROW_BYTES or kv_cache.size(-2) != kv.size(1):
    raise ValueError(f"{name}: kv must be [T, Hkv, {_DS_NOPE + _DS_ROPE}] and kv_cache [num_rows, Hkv, {_DS_ROW_BYTES}] or [num_pages, page_size, Hkv, "
                     f"{_DS_ROW_BYTES}] of the same Hkv, got {tuple(kv.shape)} and {tuple(kv_cache.shape)}")
  if slots.dtype != torch.int32 or slots.dim() != 1 or slots.numel() != kv.size(0):
    raise ValueError(f"{name}: slots must be an int32 tensor [T={kv.size(0)}], got {slots.dtype} {tuple(slots.shape)}")
  if kv.device != kv_cache.device or slots.device != kv_cache.device:
    raise ValueError(f"{name}: kv_cache / kv / slots must be on one device, got {kv_cache.device}, {kv.device}, {slots.device}")
  if kv_cache.stride(-1) != 1 or kv_cache.numel() == 0:
    raise ValueError(f"{name}: kv_cache must be a non-empty pool with a contiguous last dimension")
  from . import hip

  hip.mla_sparse_ds_pool(kv_cache, name)
  torch.ops.ffpa_attn._mla_ds_store_hip(kv_cache, kv, slots)


def ffpa_attn_with_kvcache_mla_sparse_ds(
  q: torch.Tensor,
  kv_cache: torch.Tensor,
  head_dim_v: int,
  indices: torch.Tensor,
  *,
  topk_lens: "torch.Tensor | None" = None,
  softmax_scale: float = _MLA_REQUIRED,
  num_splits: int = 0,
  return_softmax_lse: bool = False,
  **unsupported,
):
  """``ffpa_attn_with_kvcache_mla_sparse`` over the 656-byte FP8 latent rows of DeepSeek-V3.2 — the format in which the engines that serve that model keep its
  cache (vLLM's ``fp8_ds_mla``, the FP8 KV layout of FlashMLA's sparse decode; ``pack_latent_rows_ds`` says it byte by byte): ``kv_cache`` is ``torch.uint8``,
  ``[num_rows, Hkv, 656]`` or a page pool ``[num_pages, page_size, Hkv, 656]`` with evenly spaced pages; any other dtype (``TypeError``) or last dimension
  (``ValueError``) is refused.  ``q`` and the output are bf16 (fp16 ``q``: ``TypeError`` — the rotary columns of a row are bf16 and are read as they are).  The rows
  are read where they lie: the kernel is the sparse FP8 kernel's build whose pieces are a 16-byte and a 4-byte register load at the gathered offsets, dequantised
  — code x the scale of its 128 columns, rounded once to bf16 — on their way into LDS; no unpacked scratch pool, no gathered copy.  Nothing is folded into the
  softmax scale: the call returns THE BITS of ``ffpa_attn_with_kvcache_mla_sparse(q, unpack_latent_rows_ds(kv_cache), ...)``.

  ``indices`` / ``topk_lens`` and their safety rules (entries at and past the count are never turned into an address — by the scale's load as little as by the
  codes' —, entries in front of it are clamped into the pool), the required ``softmax_scale``, the ``(576, 512)`` build, ``num_splits``, the returns (``out [T, Hq,
  head_dim_v]``, fp32 ``lse [Hq, T]``) and the one-graph call are ``ffpa_attn_with_kvcache_mla_sparse``'s.  The pool's own rules (``ValueError`` before any
  launch): slot and head strides are multiples of 16 bytes, slots at least 656 bytes apart (a padded slot stride is fine), the base 16-byte aligned, and the rows
  of a latent head span at most 2^31 bytes — about 3.27 M contiguous rows.  No ``kv=``: the step's rows are written by slot, ``store_latent_rows_ds``.  Not
  served: fp16 ``q``, ue8m0 / power-of-two scale variants of the row, this layout in the dense latent call and the tree call, ``-1`` holes inside an index row
  (``compact_topk_indices``)."""
  name = "ffpa_attn_with_kvcache_mla_sparse_ds"
  if unsupported:
    raise NotImplementedError(f"{name} does not support: {', '.join(sorted(unsupported))} (no causal flag — the indexer has chosen visible keys —, no kv= append, "
                              "no window, soft-cap, tree mask, rotary tables, ALiBi, batch index or leftpad over the sparse latent call)")
  T, Hq = _mla_sparse_check(name, q, kv_cache, head_dim_v, indices, topk_lens, softmax_scale, num_splits, ds=True)
  from . import hip  # noqa: F401  (registers the ffpa_attn ops)

  if T == 0:
    out = q.new_empty((0, Hq, head_dim_v))
    return (out, q.new_empty((Hq, 0), dtype=torch.float32)) if return_softmax_lse else out
  out, lse = torch.ops.ffpa_attn._mla_sparse_ds_fwd_hip(q, kv_cache, head_dim_v, indices, topk_lens, float(softmax_scale), num_splits)
  return (out, lse) if return_softmax_lse else out


def ffpa_attn_varlen_with_kvcache(
  q: torch.Tensor,
  k_cache: torch.Tensor,
  v_cache: torch.Tensor,
  cu_seqlens_q: torch.Tensor,
  max_seqlen_q: int,
  cache_seqlens: torch.Tensor,
  block_table: torch.Tensor | None = None,
  k: torch.Tensor | None = None,
  v: torch.Tensor | None = None,
  rotary_cos: torch.Tensor | None = None,
  rotary_sin: torch.Tensor | None = None,
  positions: torch.Tensor | None = None,
  *,
  softmax_scale: float | None = None,
  causal: bool = False,
  window_size: tuple = (-1, -1),
  softcap: float = 0.0,
  rotary_interleaved: bool = True,
  num_splits: int = 0,
  return_softmax_lse: bool = False,
):
  """``ffpa_attn_with_kvcache`` for a RAGGED step — the batch of a continuous-batching engine with chunked prefill: a prompt chunk of hundreds of tokens, a few
  speculative verifications of 3 - 5 and dozens of one-token decodes in ONE call; FlashAttention's ``flash_attn_varlen_func(..., seqused_k=, block_table=)`` plus
  its cache append.  ``q [T, Hq, D]`` holds every sequence's query tokens packed by ``cu_seqlens_q`` (int32 ``[B + 1]``, on the device, unit stride: sequence b
  owns rows ``cu_seqlens_q[b] ... cu_seqlens_q[b + 1]``, ``Sq_b`` of them; empty sequences are legal anywhere).  ``max_seqlen_q`` (a host int) is a CONTRACT, as
  in ``ffpa_attn_varlen_func``: every ``Sq_b <= max_seqlen_q``; it is not checked (that would need a host read).  ``cache_seqlens`` (int32 ``[B]``, on the
  device, required): the keys each sequence's cache holds BEFORE this call's append.  The caches, ``block_table``, dtypes, layouts and strides are
  ``ffpa_attn_with_kvcache``'s — B comes from ``cu_seqlens_q``, a contiguous cache is ``[B, capacity, Hkv, D]``.

  ``k`` / ``v [T, Hkv, D]`` (packed by the same ``cu_seqlens_q``: the step's new keys are its query tokens): ONE launch in front of the attention launch
  (``ffpa_attn::_kvcache_append_varlen_hip``; every token row finds its sequence by a binary search of ``cu_seqlens_q`` on the device) writes key i of sequence b
  in place at cache position ``max(cache_seqlens[b], 0) + i``, positions at or past the capacity dropped.  With ``rotary_cos`` / ``rotary_sin`` (they require
  ``k`` / ``v``) the keys are stored rotated and a rotated copy of q attends — key i at position ``cache_seqlens[b] + i``, query token i at the same position
  under ``causal``, at ``cache_seqlens[b]`` otherwise (``ffpa_attn_with_kvcache``'s rule).  ``positions`` (int32 ``[T]``, on q's device, unit stride; requires
  the rotary tables; ``TypeError`` for another dtype, ``ValueError`` for another shape): key AND query token of row t rotate at ``positions[t]`` instead — the key
  is still written at its slot.  This is the tree-draft case, where a node's position is its depth and not its slot.  Positions are clamped to
  ``[0, seqlen_ro - 1]``.  On a uniform batch the append writes the bytes ``ffpa_attn_with_kvcache``'s does.

  Attention for sequence b runs over ``L_b`` keys — ``min(max(cache_seqlens[b], 0) + Sq_b, capacity)`` with ``k`` / ``v``, else ``cache_seqlens[b]`` clamped to
  ``[0, capacity]`` — with query token i at ``pos_i = i + L_b - Sq_b`` (bottom-right aligned per sequence).  ``causal``, ``window_size`` and ``softcap`` mean what
  they mean in ``ffpa_attn_with_kvcache``, ``_window`` and ``_softcap`` (and raise what those raise): ``softcap > 0`` takes the soft-capping launch, otherwise a
  window other than ``(-1, -1)`` the window launch, otherwise the paged launch — or the packed ``seqused_k`` launch for a contiguous cache.  The attention
  kernels are those calls' kernels, which read ``cu_seqlens_q`` and the key lengths per sequence on the device.  GQA row packing stays a launch-wide decision
  (``Hq / Hkv x max_seqlen_q`` fits a row tile): the decodes of a batch that also holds a long chunk run unpacked.  A row that sees no key returns O = 0,
  LSE = -inf.  ``cache_seqlens`` is not advanced.  There is no tree mask here.

  Returns ``out [T, Hq, D]`` — and, with ``return_softmax_lse``, the fp32 ``lse [Hq, T]`` (the layout of ``ffpa_attn_varlen_func``).  Rows at or past
  ``cu_seqlens_q[B]`` (padding: T may exceed it) are unspecified, and nothing is appended for them.  ``T == 0`` returns empty tensors and launches nothing.
  Nothing is read back to the host: the call captures into one HIP graph, and a replay follows ``q``, ``cu_seqlens_q`` (same T, same bound), ``cache_seqlens``,
  ``block_table`` and ``positions`` written in place.  Inference only: a tensor that requires grad raises ``NotImplementedError``."""
  softcap = _softcap_arg(softcap)
  left, right = _window_arg(window_size)
  ragged = (cu_seqlens_q, max_seqlen_q, positions)
  B, capacity, lens, scale = _kv_check(_RAGGED, q, k_cache, v_cache, k, v, rotary_cos, rotary_sin, cache_seqlens, block_table, softmax_scale, num_splits, ragged=ragged)
  T, Hq, D = q.shape
  if T == 0:
    out = q.new_empty((0, Hq, D))
    return (out, torch.empty((Hq, 0), dtype=torch.float32, device=q.device)) if return_softmax_lse else out
  family = ("softcap", softcap, left, right) if softcap > 0.0 else ("window", left, right) if (left, right) != (-1, -1) else ("plain",)
  o, lse = _kv_step(family, q, k_cache, v_cache, k, v, rotary_cos, rotary_sin, rotary_interleaved, lens, block_table, B, capacity, scale, causal, num_splits,
                    return_softmax_lse, ragged)
  return (o, lse) if return_softmax_lse else o


# ---- ragged query batches over the MLA latent cache: ffpa_attn_varlen_with_kvcache_mla
def ffpa_attn_varlen_with_kvcache_mla(
  q: torch.Tensor,
  kv_cache: torch.Tensor,
  head_dim_v: int,
  cu_seqlens_q: torch.Tensor,
  max_seqlen_q: int,
  cache_seqlens: torch.Tensor,
  block_table: torch.Tensor | None = None,
  *,
  kv: torch.Tensor | None = None,
  softmax_scale: float = _MLA_REQUIRED,
  causal: bool = False,
  num_splits: int = 0,
  return_softmax_lse: bool = False,
  **unsupported,
):
  """``ffpa_attn_with_kvcache_mla`` for a RAGGED step — the batch of a continuous-batching engine that serves an MLA model: MTP / speculative verification leaves
  1 - 4 tokens per sequence, a different count after every accept step, and a short extend chunk rides with dozens of one-token decodes.  ``q [T, Hq, D]`` holds
  every sequence's query tokens packed by ``cu_seqlens_q`` (int32 ``[B + 1]``, on the device, unit stride: sequence b owns rows ``cu_seqlens_q[b] ...
  cu_seqlens_q[b + 1]``, ``Sq_b`` of them; empty sequences are legal anywhere).  ``max_seqlen_q`` (a host int) is a CONTRACT, as in
  ``ffpa_attn_varlen_with_kvcache``: every ``Sq_b <= max_seqlen_q``; it is not checked (that would need a host read).  ``cache_seqlens`` (int32 ``[B]``, on the
  device, required): the latent rows each sequence's cache holds BEFORE this call's append.  ``kv_cache``, ``head_dim_v``, ``block_table``, the ``(D,
  head_dim_v)`` build list, the required ``softmax_scale`` (``TypeError``) and the contiguous cache (``[B, capacity, Hkv, D]``, ``capacity % 64 == 0``, served as
  one page per sequence through the identity table) are ``ffpa_attn_with_kvcache_mla``'s — B comes from ``cu_seqlens_q``.

  ``kv [T, Hkv, D]`` (packed by the same ``cu_seqlens_q``: the step's new latent rows are its query tokens): ONE launch in front of the attention launch
  (``ffpa_attn::_mla_append_varlen_hip``; every token row finds its sequence by a binary search of ``cu_seqlens_q`` on the device) writes row i of sequence b in
  place at cache position ``max(cache_seqlens[b], 0) + i``, every element once, positions at or past the capacity dropped.  No rotary and no ``positions``:
  rotate ``q_pe`` / ``k_pe`` before the call.

  Attention for sequence b runs over ``L_b`` keys — ``min(max(cache_seqlens[b], 0) + Sq_b, capacity)`` with ``kv``, else ``cache_seqlens[b]`` clamped to
  ``[0, capacity]`` — with query token i at ``pos_i = i + L_b - Sq_b`` (bottom-right aligned per sequence) under ``causal``.  The ``Hq / Hkv`` heads x ``Sq_b``
  tokens of a sequence are the rows of ITS ``ceil(Hq / Hkv * Sq_b / 64)`` tiles; when at least three quarters of the grid that ``max_seqlen_q`` would size find no
  row, the launch is sized by the rows there are (``ceil(Hq / Hkv * T / 64) + B`` slots per latent head).  Packing and the non-temporal fetch stay launch-wide
  decisions.  A row that sees no key returns O = 0, LSE = -inf.  ``cache_seqlens`` is not advanced.

  Returns ``out [T, Hq, head_dim_v]`` — and, with ``return_softmax_lse``, the fp32 ``lse [Hq, T]``.  Rows at or past ``cu_seqlens_q[B]`` (padding: T may exceed
  it) are unspecified, and nothing is appended for them.  ``T == 0`` returns empty tensors and launches nothing.  Nothing is read back to the host: the step
  (append + attention + the split launch's merge) captures into one HIP graph, and a replay follows ``q``, ``kv``, ``cu_seqlens_q`` (same T, same bound),
  ``cache_seqlens`` and ``block_table`` written in place.  Inference only: a tensor that requires grad raises ``NotImplementedError``.  NOT served here, each
  raises ``NotImplementedError`` naming the keyword: ``window_size``, ``softcap``, ``tree_mask``, shared-prefix cascades, ``rotary_cos`` / ``rotary_sin`` /
  ``positions``, ALiBi, ``cache_batch_idx`` / ``cache_leftpad``.  FP8 latents are a dtype error HERE: a ``torch.float8_e4m3fn`` cache is
  ``ffpa_attn_varlen_with_kvcache_mla_fp8``'s."""
  name = "ffpa_attn_varlen_with_kvcache_mla"
  if unsupported:
    raise NotImplementedError(f"{name} does not support: {', '.join(sorted(unsupported))} (no window, soft-cap, tree mask, cascade, rotary tables or positions, "
                              "ALiBi, batch index or leftpad over the latent cache: rotate q_pe / k_pe before the call)")
  capacity, lens = _mla_check(name, q, kv_cache, head_dim_v, kv, cache_seqlens, block_table, softmax_scale, num_splits, ragged=(cu_seqlens_q, max_seqlen_q))
  return _mla_step_varlen(name, "mla", None, q, kv_cache, head_dim_v, cu_seqlens_q, max_seqlen_q, kv, lens, block_table, capacity, softmax_scale, causal, num_splits,
                          return_softmax_lse)


# ---- ragged query batches under a tree mask over the MLA latent cache: ffpa_attn_varlen_with_kvcache_mla_tree
def ffpa_attn_varlen_with_kvcache_mla_tree(
  q: torch.Tensor,
  kv_cache: torch.Tensor,
  head_dim_v: int,
  cu_seqlens_q: torch.Tensor,
  max_seqlen_q: int,
  cache_seqlens: torch.Tensor,
  block_table: torch.Tensor | None = None,
  *,
  tree_mask: torch.Tensor,
  kv: torch.Tensor | None = None,
  softmax_scale: float = _MLA_REQUIRED,
  num_splits: int = 0,
  return_softmax_lse: bool = False,
  **unsupported,
):
  """``ffpa_attn_with_kvcache_mla_tree`` for a RAGGED step: the sequences of a continuous-batching engine bring draft trees of different sizes (and plain decodes:
  a tree of one node).  ``q [T, Hq, D]``, ``cu_seqlens_q``, the ``max_seqlen_q`` contract, ``cache_seqlens``, ``kv [T, Hkv, D]`` and its per-token append launch,
  ``kv_cache``, ``head_dim_v``, ``block_table``, the REQUIRED ``softmax_scale``, the row chunks, the compact grid, ``num_splits`` and the returns (``out [T, Hq,
  head_dim_v]``, fp32 ``lse [Hq, T]``; rows at or past ``cu_seqlens_q[B]`` unspecified) are ``ffpa_attn_varlen_with_kvcache_mla``'s — B comes from
  ``cu_seqlens_q``.  ``tree_mask``: bool ``[W, W]`` or ``[B, W, W]``, or the int64 words ``[B | 1, W]`` of ``pack_tree_mask``, ``max_seqlen_q <= W <= 64``;
  sequence b with ``n_b`` tokens uses the top-left ``n_b x n_b`` of its mask.  With ``L_b`` the rows attention runs over (``min(max(cache_seqlens[b], 0) + n_b,
  capacity)`` with ``kv``, else ``cache_seqlens[b]`` clamped to ``[0, capacity]``), query token i of sequence b sees

  * row ``p`` for every ``p < L_b - n_b`` (the prefix), and
  * row ``L_b - n_b + j`` iff ``tree_mask[b, i, j]``; draft positions below 0 do not exist.

  A row that sees nothing returns O = 0, LSE = -inf.  ``T == 0`` returns empty tensors and launches nothing.  Nothing is read back to the host: the step (append +
  attention + the split launch's merge) captures into one HIP graph, and a replay follows ``q``, ``kv``, the mask words, ``cu_seqlens_q`` (same T, same bound),
  ``cache_seqlens`` and ``block_table`` written in place.  Inference only.  NOT served here, each raises ``NotImplementedError`` naming the keyword: ``causal`` (the
  mask says it), ``window_size``, ``softcap``, shared-prefix cascades, ``rotary_cos`` / ``rotary_sin`` / ``positions``, ALiBi, ``cache_batch_idx`` /
  ``cache_leftpad``, masks over the prefix, more than 64 draft tokens per sequence and FP8 latents (a dtype error)."""
  name = "ffpa_attn_varlen_with_kvcache_mla_tree"
  if unsupported:
    raise NotImplementedError(f"{name} does not support: {', '.join(sorted(unsupported))} ({_MLA_TREE_UNSERVED}; no positions)")
  capacity, lens = _mla_check(name, q, kv_cache, head_dim_v, kv, cache_seqlens, block_table, softmax_scale, num_splits, ragged=(cu_seqlens_q, max_seqlen_q))
  if isinstance(tree_mask, torch.Tensor) and tree_mask.requires_grad and torch.is_grad_enabled():
    raise NotImplementedError(f"{name} is inference only: tree_mask requires grad and there is no backward")
  return _mla_step_varlen(name, "tree", tree_mask, q, kv_cache, head_dim_v, cu_seqlens_q, max_seqlen_q, kv, lens, block_table, capacity, softmax_scale, False, num_splits,
                          return_softmax_lse)


def ffpa_attn_varlen_with_kvcache_mla_tree_fp8(
  q: torch.Tensor,
  kv_cache: torch.Tensor,
  head_dim_v: int,
  cu_seqlens_q: torch.Tensor,
  max_seqlen_q: int,
  cache_seqlens: torch.Tensor,
  block_table: torch.Tensor | None = None,
  *,
  kv_scale: float = 1.0,
  tree_mask: torch.Tensor,
  kv: torch.Tensor | None = None,
  softmax_scale: float = _MLA_REQUIRED,
  num_splits: int = 0,
  return_softmax_lse: bool = False,
  **unsupported,
):
  """``ffpa_attn_varlen_with_kvcache_mla_tree`` over an FP8 latent cache: the ragged step (``q [T, Hq, D]`` packed by ``cu_seqlens_q``, draft trees of different
  sizes) of ``ffpa_attn_with_kvcache_mla_tree_fp8`` — ``kv_cache`` is ``torch.float8_e4m3fn`` under the per-tensor ``kv_scale`` (a host float), ``q``, ``kv [T, Hkv,
  D]`` and the output are bf16 or fp16, and ``kv`` is quantised by the ragged FP8 append as ``quantize_latent_rows(kv, kv_scale)``.  Everything else is
  ``ffpa_attn_varlen_with_kvcache_mla_tree``'s; every sequence's rows are the bits of the uniform FP8 tree call on that sequence alone."""
  name = "ffpa_attn_varlen_with_kvcache_mla_tree_fp8"
  if unsupported:
    raise NotImplementedError(f"{name} does not support: {', '.join(sorted(unsupported))} ({_MLA_TREE_UNSERVED}; no positions)")
  from . import hip  # (registers the ffpa_attn ops)

  kv_scale = hip.check_kv_scale(kv_scale, name)
  capacity, lens = _mla_check(name, q, kv_cache, head_dim_v, kv, cache_seqlens, block_table, softmax_scale, num_splits, fp8=True, ragged=(cu_seqlens_q, max_seqlen_q))
  if isinstance(tree_mask, torch.Tensor) and tree_mask.requires_grad and torch.is_grad_enabled():
    raise NotImplementedError(f"{name} is inference only: tree_mask requires grad and there is no backward")
  return _mla_step_varlen(name, "tree_fp8", (tree_mask, kv_scale), q, kv_cache, head_dim_v, cu_seqlens_q, max_seqlen_q, kv, lens, block_table, capacity, softmax_scale,
                          False, num_splits, return_softmax_lse)


# ---- cascade (shared-prefix) attention: ffpa_attn_with_kvcache_cascade
# cascade=None takes the cascade where the K + V re-reads it saves — (B - 1) * P keys x Hkv x D x 2 (K and V) x 2 bytes, the copies of the prefix the plain
# launch streams for sequences 1 .. B - 1 — reach _CASCADE_MIN_SAVED_BYTES.  Fitted to the interleaved A/B of tools/gpu_cascade_ab.py on MI355X
# (profiles/r09_cascade_ab.json, "grid" rows: paged, page 64, D 512 GQA 32 / 8 and D 1024 GQA 16 / 4, B 4 / 16 / 64, Sq 1 / 4, P 2k / 8k / 32k, suffixes
# 128 ... 2k).  All 24 shapes that save >= 1536 MiB won, in graph replay AND launched eagerly (1.16 ... 9.0 x).  Of the 12 that save <= 480 MiB, 11 lost in at
# least one of the two (0.41 ... 1.00 x: the cascade's extra launches, ~ 25 us replayed and ~ 80 us from Python, outweigh what the Infinity Cache leaves of the
# re-reads); the twelfth, B 16 Sq 1 P 2k D 512 (480 MiB), won narrowly (1.19 x / 1.03 x) while its Sq 4 twin lost (0.89 x / 0.85 x).  The threshold sits
# between 480 and 1536 MiB.  The rule stays inside what was measured: paged caches, GQA groups of 4 or more, Sq <= 4, D >= 512.  Page size and groups above 4
# are an extrapolation along the saved-bytes axis, checked by the "check" rows of the same profile (page 256; group 8).  Contiguous caches, MHA / small
# groups, Sq > 4 and D < 512 were not measured and stay plain under None; cascade=True forces the cascade there.
_CASCADE_MIN_SAVED_BYTES = 1 << 30
_CASCADE_MAX_SEQLEN_Q = 4
_CASCADE_MIN_HEAD_DIM = 512
_CASCADE_MIN_GROUP = 4


def cascade_rule(batch: int, seqlen_q: int, heads_q: int, heads_kv: int, head_dim: int, shared_prefix_len: int, page_size: int) -> bool:
  """The host-side rule of ``ffpa_attn_with_kvcache_cascade(cascade=None)``: True where the cascade (prefix pass + suffix pass + merge) is expected faster than
  the plain launch — the re-reads it saves reach 1 GiB — inside the measured envelope (``page_size`` > 0: a paged cache; ``heads_q / heads_kv`` >= 4; Sq <= 4;
  D >= 512).  A batch of one, or no shared prefix, is always plain."""
  if batch <= 1 or shared_prefix_len <= 0:
    return False
  if seqlen_q < 1 or seqlen_q > _CASCADE_MAX_SEQLEN_Q or head_dim < _CASCADE_MIN_HEAD_DIM:
    return False
  if page_size <= 0 or heads_kv <= 0 or heads_q // heads_kv < _CASCADE_MIN_GROUP:
    return False
  saved = (batch - 1) * shared_prefix_len * heads_kv * head_dim * 2 * 2
  return saved >= _CASCADE_MIN_SAVED_BYTES


def _merge(o_a, lse_a, o_b, lse_b):
  return torch.ops.ffpa_attn._merge_states_hip(o_a, lse_a, o_b, lse_b)


def ffpa_merge_attn_states(o_a: torch.Tensor, lse_a: torch.Tensor, o_b: torch.Tensor, lse_b: torch.Tensor):
  """Merge two attention states of the same queries over two disjoint key sets (FlashInfer's / vLLM's ``merge_attn_states``): ``o_a`` / ``o_b [T, H, D]`` (bf16 or
  fp16, one dtype; D a multiple of 8 up to 1024) with their fp32 ``lse_a`` / ``lse_b [H, T]`` (natural log; the layout ``ffpa_attn_varlen_func`` returns; any head
  stride) -> ``(o [T, H, D], lse [H, T])``, the attention over the union of the key sets.  Per row, in fp32: ``m = max(lse_a, lse_b)``, ``w = exp(lse - m)``,
  ``o = (w_a o_a + w_b o_b) / (w_a + w_b)`` rounded once, ``lse = m + ln(w_a + w_b)``.  A side whose LSE is -inf contributes nothing (a NaN in its O does not
  leak); both -inf gives ``o = 0``, ``lse = -inf``.  One HIP launch, nothing read back to the host.  Inference only: a tensor that requires grad (with grad
  mode on) raises ``NotImplementedError``."""
  from . import hip

  for name, t in (("o_a", o_a), ("lse_a", lse_a), ("o_b", o_b), ("lse_b", lse_b)):
    if isinstance(t, torch.Tensor) and t.requires_grad and torch.is_grad_enabled():
      raise NotImplementedError(f"ffpa_merge_attn_states is inference only: {name} requires grad and there is no backward")
  hip.check_merge_states(o_a, lse_a, o_b, lse_b)
  return _merge(o_a, lse_a, o_b, lse_b)


def ffpa_attn_with_kvcache_cascade(
  q: torch.Tensor,
  k_cache: torch.Tensor,
  v_cache: torch.Tensor,
  k: torch.Tensor | None = None,
  v: torch.Tensor | None = None,
  rotary_cos: torch.Tensor | None = None,
  rotary_sin: torch.Tensor | None = None,
  cache_seqlens: "int | torch.Tensor | None" = None,
  block_table: torch.Tensor | None = None,
  *,
  shared_prefix_len: int,
  softmax_scale: float | None = None,
  causal: bool = False,
  rotary_interleaved: bool = True,
  num_splits: int = 0,
  return_softmax_lse: bool = False,
  cascade: "bool | None" = None,
):
  """``ffpa_attn_with_kvcache`` for a batch whose sequences share their first ``shared_prefix_len`` (P) keys — parallel sampling, beam search, a shared system
  prompt under prefix caching — as CASCADE attention: the prefix is read once per KV head for the whole batch instead of once per sequence.  Three launches
  (four with ``k`` / ``v``), nothing read back to the host, so a call captures into one HIP graph:

  1. (with ``k`` / ``v``) the append of ``ffpa_attn_with_kvcache`` on the full table: its rotated q and post-append lengths feed both passes;
  2. PREFIX pass: all ``B * Sq`` query tokens as ONE sequence against keys ``[0, P)`` of sequence 0 — pages ``block_table[0, :P / page_size]``, or rows
     ``[0, P)`` of ``k_cache[0]`` — not causal;
  3. SUFFIX pass: the plain launch on ``block_table[:, P / page_size:]`` (a contiguous cache: every slab from row P on, no copy) with lengths
     ``max(len_b - P, 0)`` computed on the device, under the caller's ``causal`` (exact: the alignment is bottom-right);
  4. the merge of the two (O, LSE) states (``ffpa_merge_attn_states``).

  Everything else — arguments, shapes, returns, checks — is ``ffpa_attn_with_kvcache``'s.  Contracts (not checked: they would need a host read):
  keys ``[0, P)`` are the same for every sequence (the same pages in every row of ``block_table``, the same rows in every slab) and are read from sequence 0
  only; every sequence holds at least P keys; appended keys land at or past P (a write into shared pages is the caller's race, as in FlashAttention); under
  ``causal`` every sequence's suffix holds at least its ``Sq`` query tokens.  A paged cache needs P to be a multiple of ``page_size``.

  ``cascade``: False = exactly ``ffpa_attn_with_kvcache`` (the same launch, the same bits); True = the cascade (P = 0, or P = the capacity, leaves one key set:
  the plain launch); None = ``cascade_rule`` — measured on MI355X, it takes the cascade only where it won.  The cascade differs from the plain launch by
  rounding only: two normalised partial states merged in fp32 instead of one pass."""
  if isinstance(shared_prefix_len, bool) or not isinstance(shared_prefix_len, int):
    raise TypeError(f"ffpa_attn_with_kvcache_cascade: shared_prefix_len must be an int, got {type(shared_prefix_len).__name__}")
  if shared_prefix_len < 0:
    raise ValueError(f"ffpa_attn_with_kvcache_cascade: shared_prefix_len must be non-negative, got {shared_prefix_len}")
  if cascade is not None and not isinstance(cascade, bool):
    raise TypeError(f"ffpa_attn_with_kvcache_cascade: cascade must be True, False or None, got {cascade!r}")
  B, capacity, lens, scale = _kv_check(_UNIFORM, q, k_cache, v_cache, k, v, rotary_cos, rotary_sin, cache_seqlens, block_table, softmax_scale, num_splits)
  P = shared_prefix_len
  Sq, Hq, D = q.shape[1:]
  Hkv = k_cache.size(2)
  page_size = k_cache.size(1) if block_table is not None else 0
  if P > capacity:
    raise ValueError(f"ffpa_attn_with_kvcache_cascade: shared_prefix_len ({P}) exceeds the cache capacity ({capacity})")
  if block_table is not None and P % page_size != 0:
    raise ValueError(f"ffpa_attn_with_kvcache_cascade: shared_prefix_len ({P}) must be a multiple of page_size ({page_size}) in a paged cache")
  if cascade is False:
    return ffpa_attn_with_kvcache(q, k_cache, v_cache, k, v, rotary_cos, rotary_sin, cache_seqlens, block_table=block_table, softmax_scale=softmax_scale,
                                  causal=causal, rotary_interleaved=rotary_interleaved, num_splits=num_splits, return_softmax_lse=return_softmax_lse)
  use = cascade_rule(B, Sq, Hq, Hkv, D, P, page_size) if cascade is None else True
  use = use and 0 < P < capacity and B * Sq > 0
  if not use:
    o, lse = _kv_step(("plain",), q, k_cache, v_cache, k, v, rotary_cos, rotary_sin, rotary_interleaved, lens, block_table, B, capacity, scale, causal, num_splits,
                      return_softmax_lse)
  else:
    if k is not None:
      q, lens = _kv_append(q, k_cache, v_cache, k, v, rotary_cos, rotary_sin, rotary_interleaved, causal, lens, block_table)
    o, lse = _cascade(q, k_cache, v_cache, lens, block_table, capacity, P, scale, causal, num_splits)
  return _kv_unpack(o, lse, q, return_softmax_lse)


def _cascade(q, k_cache, v_cache, seqused, block_table, capacity, P, scale, causal, num_splits):
  """The prefix pass, the suffix pass and the merge -> packed ``(o [B * Sq, Hq, D], lse [Hq, B * Sq])``.  0 < P < capacity, B * Sq > 0."""
  B, Sq, Hq, D = q.shape
  dev = q.device
  T = B * Sq
  qp = q.reshape(T, Hq, D)
  # the prefix pass: one sequence of T query tokens against keys [0, P) of sequence 0 (lengths and boundaries made on the device: nothing crosses to the host)
  cu_pre = torch.arange(0, 2 * T, T, dtype=torch.int32, device=dev)
  # the suffix pass: keys from P on, lengths len_b - P (clamped to what the suffix can hold, as the plain launch clamps to the capacity)
  used_suf = (seqused - P).clamp(0, capacity - P)
  cu_q = torch.arange(0, (B + 1) * Sq, Sq, dtype=torch.int32, device=dev)
  if block_table is not None:
    pp = P // k_cache.size(1)
    used_pre = torch.full((1,), P, dtype=torch.int32, device=dev)
    o_p, lse_p = _kv_launch(("plain",), qp, k_cache, v_cache, cu_pre, None, used_pre, block_table[:1, :pp], T, P, scale, False, num_splits)
    o_s, lse_s = _kv_launch(("plain",), qp, k_cache, v_cache, cu_q, None, used_suf, block_table[:, pp:], Sq, capacity - P, scale, causal, num_splits)
  else:
    cu_kp = torch.arange(0, 2 * P, P, dtype=torch.int32, device=dev)
    o_p, lse_p = _kv_launch(("plain",), qp, k_cache[0, :P], v_cache[0, :P], cu_pre, cu_kp, None, None, T, P, scale, False, num_splits)
    # sequence b's suffix: rows b * capacity + P ... of the plain launch's view — the same boundaries, shifted by P rows
    kp, vp, cu_k = _kv_view(k_cache, v_cache, B, capacity)
    o_s, lse_s = _kv_launch(("plain",), qp, kp[P:], vp[P:], cu_q, cu_k, used_suf, None, Sq, capacity - P, scale, causal, num_splits)
  return _merge(o_p, lse_p, o_s, lse_s)


# ---- shared-prefix (cascade) attention over the MLA latent cache: ffpa_attn_with_kvcache_mla_cascade / ffpa_attn_with_kvcache_mla_cascade_fp8
# cascade=None, measured on MI355X (profiles/r26_mla_cascade.md, tools/gpu_mla_cascade_ab.py; "fit" rows: page 64, Hq 16 / 128 on one latent head, B 16 / 64 as one
# group and B 64 as 8 groups of 8, P 2k / 8k / 32k, suffixes 128 / 2k, 1 token and 4 tokens causal).  The latent step is bound by its tiles, not by its bytes: what
# the cascade buys is tiles FILLED — at Hq 16, one token, a 64-row tile of the plain call holds 16 live rows, and the prefix pass packs four sequences into it.  So
# the only class that won is Hq 16 x 1 token: at B x P = 2^21 sequence-keys (B 64, P 32k: 4 shapes) and at 2^20 (B 64 x 16k, B 128 x 8k) it won replayed from a
# graph AND launched eagerly (1.96 ... 2.53 x), in groups of 64, 8 and 4 sequences alike (4 x 16 rows fill a tile); at 2^19 (B 64 x 8k, B 16 x 32k) it won
# replayed (1.32 ... 1.46 x) and LOST eagerly (0.60 ... 0.95 x: five launches from Python cost ~ 135 us, the plain step 110 ... 130 us), below that it lost both.
# With 4 tokens (64 rows: the tiles are full) it lost everywhere at Hq 16 (0.56 ... 0.93 x), and at Hq 128 it lost (0.57 ... 0.96 x) except at P 32k in ONE group
# (1.02 ... 1.22 x, both ways) — too narrow a win to build a class on: it stays plain.  The rule takes the measured winners; the "check" rows of the same profile
# confirm it off the grid (B 32 ... 256, P 8k ... 64k, 16 ... 96 sequences per group, pages of 128, one FP8 row: 2.16 ... 2.67 x, both ways).  Everything else was
# either measured as a loss or NOT MEASURED and stays plain under None: more than one latent head, other head counts, Sq > 1 at Hq < 16, groups of fewer than 4
# sequences; cascade=True forces the cascade there.
_MLA_CASCADE_HEADS_Q = 16             # r26_mla_cascade: query heads on the one latent head, one token: 16 live rows of a tile's 64
_MLA_CASCADE_MIN_SEQ_KEYS = 1 << 20    # r26_mla_cascade: batch x shared_prefix_len; 2^19 lost eagerly, 2^20 won both
_MLA_CASCADE_MIN_GROUP_SEQS = 4        # r26_mla_cascade: sequences per group (batch / num_groups), the smallest measured


def mla_cascade_rule(batch: int, seqlen_q: int, heads_q: int, heads_kv: int, shared_prefix_len: int, num_groups: int = 1) -> bool:
  """The host-side rule of ``ffpa_attn_with_kvcache_mla_cascade(cascade=None)`` for a host-int ``shared_prefix_len``: True where the cascade (plan + prefix pass +
  suffix pass + merge) was measured faster than the plain latent launch on MI355X, replayed from a graph AND launched eagerly (profiles/r26_mla_cascade.md): one
  latent head under 16 query heads, one token, ``batch * shared_prefix_len >= 2^20`` sequence-keys and on average 4 or more sequences per group.  Everything else
  — measured as a loss, or not measured — is plain."""
  if num_groups < 1 or batch <= num_groups or shared_prefix_len <= 0 or seqlen_q < 1 or heads_kv <= 0 or heads_q < heads_kv:
    return False
  if heads_kv != 1 or heads_q != _MLA_CASCADE_HEADS_Q or seqlen_q != 1:
    return False
  if batch < _MLA_CASCADE_MIN_GROUP_SEQS * num_groups:
    return False
  return batch * shared_prefix_len >= _MLA_CASCADE_MIN_SEQ_KEYS


def _mla_cascade(name, fp8, kv_scale, q, kv_cache, head_dim_v, shared_prefix_len, cu_group_seqs, max_group_seqs, kv, cache_seqlens, block_table, softmax_scale, causal,
                 num_splits, return_softmax_lse, cascade):
  """Both cascade calls behind their names: the checks, the route (plain / cascade) and the cascade's five steps."""
  if cascade is not None and not isinstance(cascade, bool):
    raise TypeError(f"{name}: cascade must be True, False or None, got {cascade!r}")
  on_device = isinstance(shared_prefix_len, torch.Tensor)
  if not on_device:
    if isinstance(shared_prefix_len, bool) or not isinstance(shared_prefix_len, int):
      raise TypeError(f"{name}: shared_prefix_len must be an int or an int32 device tensor [groups], got {type(shared_prefix_len).__name__}")
    if shared_prefix_len < 0:
      raise ValueError(f"{name}: shared_prefix_len must be non-negative, got {shared_prefix_len}")
  capacity, lens = _mla_check(name, q, kv_cache, head_dim_v, kv, cache_seqlens, block_table, softmax_scale, num_splits, fp8=fp8)
  if block_table is None:
    raise ValueError(f"{name}: block_table is required — a contiguous latent cache has no shared pages (every sequence owns its slab); the plain call serves it")
  B, Sq, Hq, _ = q.shape
  G = 1
  if cu_group_seqs is not None:
    if not isinstance(cu_group_seqs, torch.Tensor) or cu_group_seqs.dtype != torch.int32:
      raise TypeError(f"{name}: cu_group_seqs must be an int32 tensor [groups + 1], got {getattr(cu_group_seqs, 'dtype', type(cu_group_seqs).__name__)}")
    if cu_group_seqs.dim() != 1 or cu_group_seqs.numel() < 2 or cu_group_seqs.device != q.device:
      raise ValueError(f"{name}: cu_group_seqs must be a 1-D int32 tensor [groups + 1] on q's device, got {tuple(cu_group_seqs.shape)} on {cu_group_seqs.device}")
    G = cu_group_seqs.numel() - 1
  if on_device:
    if shared_prefix_len.dtype != torch.int32:
      raise TypeError(f"{name}: a tensor shared_prefix_len must be int32, got {shared_prefix_len.dtype}")
    if tuple(shared_prefix_len.shape) != (G,) or shared_prefix_len.device != q.device:
      raise ValueError(f"{name}: a tensor shared_prefix_len must be [groups={G}] on q's device, got {tuple(shared_prefix_len.shape)} on {shared_prefix_len.device}")
  if max_group_seqs is None:
    max_group_seqs = B
  elif isinstance(max_group_seqs, bool) or not isinstance(max_group_seqs, int) or max_group_seqs < 0 or (B > 0 and max_group_seqs < 1):
    raise ValueError(f"{name}: max_group_seqs must be a host int >= 1 that bounds the sequences of every group, got {max_group_seqs!r}")
  op = "fp8" if fp8 else "mla"
  use = cascade
  if use is None:
    use = True if on_device else mla_cascade_rule(B, Sq, Hq, kv_cache.size(2), shared_prefix_len, G)
  if not use or B == 0 or Sq == 0:
    return _mla_step(name, op, kv_scale, q, kv_cache, head_dim_v, kv, lens, block_table, capacity, softmax_scale, causal, num_splits, return_softmax_lse)
  # 1. the step's latent rows into the pool, on the full table: the ragged append with Snew rows per sequence returns the post-append lengths
  if kv is not None and kv.size(1) > 0:
    Snew = kv.size(1)
    cu_new = torch.arange(0, (B + 1) * Snew, Snew, dtype=torch.int32, device=q.device)
    rows = kv.reshape(B * Snew, kv.size(2), kv.size(3))
    if fp8:
      lens = torch.ops.ffpa_attn._mla_fp8_append_varlen_hip(kv_cache, rows, kv_scale, cu_new, lens, block_table)
    else:
      lens = torch.ops.ffpa_attn._mla_append_varlen_hip(kv_cache, rows, cu_new, lens, block_table)
  # 2. the plan: effective prefixes, the groups' query boundaries, the prefix rows and the shifted suffix rows, in one launch
  cu_pre, len_pre, table_pre, table_suf, len_suf = torch.ops.ffpa_attn._mla_cascade_plan_hip(
    lens, block_table, cu_group_seqs, shared_prefix_len if on_device else None, 0 if on_device else shared_prefix_len, kv_cache.size(1), Sq, 1 if causal else 0, capacity)
  qp = q.reshape(B * Sq, Hq, q.size(3))
  cu_q = torch.arange(0, (B + 1) * Sq, Sq, dtype=torch.int32, device=q.device)
  scale = float(softmax_scale)
  # 3. the prefix pass (every group one packed sequence, not causal) and 4. the suffix pass (the caller's causal: bottom-right aligned, so exact)
  if fp8:
    o_p, lse_p = torch.ops.ffpa_attn._mla_fp8_fwd_hip(qp, kv_cache, head_dim_v, kv_scale, cu_pre, len_pre, table_pre, None, None, max_group_seqs * Sq, capacity, scale, 0,
                                                      num_splits)
    o_s, lse_s = torch.ops.ffpa_attn._mla_fp8_fwd_hip(qp, kv_cache, head_dim_v, kv_scale, cu_q, len_suf, table_suf, None, None, Sq, capacity, scale,
                                                      1 if causal else 0, num_splits)
  else:
    o_p, lse_p = torch.ops.ffpa_attn._mla_fwd_hip(qp, kv_cache, head_dim_v, cu_pre, len_pre, table_pre, None, None, max_group_seqs * Sq, capacity, scale, 0, num_splits)
    o_s, lse_s = torch.ops.ffpa_attn._mla_fwd_hip(qp, kv_cache, head_dim_v, cu_q, len_suf, table_suf, None, None, Sq, capacity, scale, 1 if causal else 0, num_splits)
  # 5. the merge of the two states
  o, lse = _merge(o_p, lse_p, o_s, lse_s)
  out = o.view(B, Sq, Hq, head_dim_v)
  if not return_softmax_lse:
    return out
  return out, lse.view(Hq, B, Sq).permute(1, 0, 2).contiguous()


def ffpa_attn_with_kvcache_mla_cascade(
  q: torch.Tensor,
  kv_cache: torch.Tensor,
  head_dim_v: int,
  *,
  shared_prefix_len: "int | torch.Tensor",
  cu_group_seqs: torch.Tensor | None = None,
  max_group_seqs: int | None = None,
  kv: torch.Tensor | None = None,
  cache_seqlens: "int | torch.Tensor",
  block_table: torch.Tensor,
  softmax_scale: float,
  causal: bool = False,
  num_splits: int = 0,
  return_softmax_lse: bool = False,
  cascade: "bool | None" = None,
):
  """``ffpa_attn_with_kvcache_mla`` for a batch whose sequences share their first keys — a shared system prompt under prefix caching, parallel sampling and
  best-of-n, RL rollouts that draw many samples per prompt — as CASCADE attention over the latent cache: the shared latent rows are read once per GROUP of
  sequences instead of once per sequence, and the prefix pass fills its 64-row tiles with the rows of several sequences at once (at ``Hq = 16``, one token, a
  tile of the plain call holds 16 live rows).  Shapes, return values, the required ``softmax_scale``, the ``(576, 512)`` build, ``cache_seqlens``, ``causal``,
  ``num_splits``, the ``kv=`` append, inference only and every argument check are ``ffpa_attn_with_kvcache_mla``'s.  ``block_table`` is REQUIRED: a contiguous
  latent cache has no shared pages (``ValueError``).

  GROUPS.  ``cu_group_seqs`` (int32 ``[G + 1]``, on the device; non-decreasing from 0 to B; not checked) cuts the batch into G groups of consecutive sequences;
  None is one group of all B; an empty group is allowed.  The shared keys of group g are read through the ``block_table`` row of its FIRST sequence only.
  ``max_group_seqs`` (a host int, default B: always safe) bounds the sequences of any one group; it sizes the prefix pass (``max_seqlen_q = max_group_seqs *
  Sq``) and is a contract like ``max_seqlen_q`` of the ragged calls — not checked; the latent launch's compact grid takes over when most of the full grid would be
  idle.

  PREFIX LENGTHS.  ``shared_prefix_len``: a non-negative host int (one length for every group) or an int32 device tensor ``[G]``.  Nothing of it is read back to
  the host; the effective prefix is made on the device::

      P_g = page_size * floor(clamp(min(shared_prefix_len[g], min over b in g of (clamp(len_b, 0, capacity) - (Sq - 1 if causal else 0))), 0, capacity) / page_size)

  with ``len_b`` the length after the append; an empty group has ``P_g = 0``.  A length that is no page multiple is rounded down, one that exceeds what some
  sequence of the group holds (or what its first causal token may see) is cut back: the call is exact for ANY lengths.  THE ONE UNCHECKED CONTRACT: pages
  ``[0, P_g / page_size)`` really are the same keys for every sequence of group g.  An append into shared pages is the caller's race.

  STEPS of the cascade, nothing read back to the host, so the whole call captures into one HIP graph and a replay follows ``cache_seqlens``, ``block_table``,
  ``cu_group_seqs`` and a tensor ``shared_prefix_len`` written in place: (1) with ``kv``, the ragged latent append on the full table; (2) ONE plan launch
  (``ffpa_attn::_mla_cascade_plan_hip``): the effective prefixes, the queries' boundaries by group, the prefix rows and every row shifted left by its group's
  prefix pages; (3) the PREFIX pass: the latent kernel on the packed q as G sequences against ``P_g`` keys, not causal; (4) the SUFFIX pass: the latent kernel on
  the shifted table with lengths ``len_b - P_g`` under the caller's ``causal`` (bottom-right aligned: exact); (5) the merge of the two (O, LSE) states
  (``ffpa_merge_attn_states``).  The cascade differs from the plain launch by rounding only; with ``P_g = 0`` it returns the plain call's bits.

  ``cascade``: False = exactly ``ffpa_attn_with_kvcache_mla`` (the same launch, the same bits, the same append); True = the cascade; None = ``mla_cascade_rule``
  when ``shared_prefix_len`` is a host int — and the CASCADE when it is a device tensor: that cannot be priced without a host read, and the caller who built
  device-side groups has asked for it.  ``B * Sq == 0`` returns the plain call's empty results.  NOT served: ragged ``q``, the tree-mask and sparse calls,
  contiguous caches."""
  return _mla_cascade("ffpa_attn_with_kvcache_mla_cascade", False, None, q, kv_cache, head_dim_v, shared_prefix_len, cu_group_seqs, max_group_seqs, kv, cache_seqlens,
                      block_table, softmax_scale, causal, num_splits, return_softmax_lse, cascade)


def ffpa_attn_with_kvcache_mla_cascade_fp8(
  q: torch.Tensor,
  kv_cache: torch.Tensor,
  head_dim_v: int,
  *,
  shared_prefix_len: "int | torch.Tensor",
  kv_scale: float = 1.0,
  cu_group_seqs: torch.Tensor | None = None,
  max_group_seqs: int | None = None,
  kv: torch.Tensor | None = None,
  cache_seqlens: "int | torch.Tensor",
  block_table: torch.Tensor,
  softmax_scale: float,
  causal: bool = False,
  num_splits: int = 0,
  return_softmax_lse: bool = False,
  cascade: "bool | None" = None,
):
  """``ffpa_attn_with_kvcache_mla_cascade`` over an FP8 latent cache: ``kv_cache`` is ``torch.float8_e4m3fn`` under the per-tensor ``kv_scale`` (a host float,
  finite and positive), ``q``, ``kv`` and the output are bf16 or fp16, ``kv`` is quantised by the append as ``quantize_latent_rows(kv, kv_scale)`` — everything
  ``ffpa_attn_with_kvcache_mla_fp8`` says of the pool.  Groups, prefix lengths, the steps, ``cascade`` and the contract are the 16-bit cascade's; both passes run
  the FP8 latent kernel, so with a power-of-two ``kv_scale`` the call returns the bits of ``ffpa_attn_with_kvcache_mla_cascade(q, kv_cache.to(q.dtype), ...,
  softmax_scale=softmax_scale * kv_scale) * kv_scale``.  ``cascade=False`` is exactly ``ffpa_attn_with_kvcache_mla_fp8``."""
  name = "ffpa_attn_with_kvcache_mla_cascade_fp8"
  from . import hip  # (registers the ffpa_attn ops)

  kv_scale = hip.check_kv_scale(kv_scale, name)
  return _mla_cascade(name, True, kv_scale, q, kv_cache, head_dim_v, shared_prefix_len, cu_group_seqs, max_group_seqs, kv, cache_seqlens, block_table, softmax_scale,
                      causal, num_splits, return_softmax_lse, cascade)
