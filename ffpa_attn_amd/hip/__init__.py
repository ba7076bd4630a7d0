"""``ffpa_attn::_fwd_hip`` — the torch-facing shim over the C-ABI HIP library.

This module is the MI355X replacement for the reference's CUDA op shim
(``src/ffpa_attn/cuda/__init__.py:57-171`` + ``cuda/_ffpa_fwd.py:6-62``):

* it loads ``libffpa_attn_hip.so`` (built in-tree by :mod:`ffpa_attn_amd.build`) with
  ``ctypes`` — the library has no torch dependency, the boundary is
  ``include/ffpa_attn.h``;
* it registers the torch.library op ``ffpa_attn::_fwd_hip`` whose first eleven
  arguments are the reference op's (``q, k, v, attn_bias, stages, acc, causal,
  softmax_scale, dropout_p, philox_seed, philox_offset``) and which returns
  ``(o, softmax_lse)`` with ``softmax_lse`` an exact-length ``[B, Hq, Nq]`` fp32 tensor
  (``cuda/__init__.py:100-112``);
* it registers a fake (meta) implementation so ``torch.compile`` can trace through.

There is NO fallback in here: if the library is missing or was not built for this GPU
the op raises ``RuntimeError`` (the reference raises the same class when ``_C`` was not
compiled, ``cuda/__init__.py:94-99``).
"""

from __future__ import annotations

import ctypes
import math
import os
import threading

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
_PKG = os.path.dirname(_HERE)
LIB_PATH = os.path.join(_PKG, "libffpa_attn_hip.so")
TEST_LIB_PATH = os.path.join(_PKG, "libffpa_attn_hip_test.so")  # product kernels + the register-staged SAFE twins (tests only)

ABI_VERSION = 7  # 5: + the packed-sequence entry points (ffpa_attn_varlen_fwd ...); 6: + KV splits inside the packed call; 7: + the paged-KV call

# enum ffpa_status (include/ffpa_attn.h)
_STATUS_EXC = {
  1: RuntimeError,  # NULL pointer
  2: TypeError,  # dtype
  3: RuntimeError,  # "headdim not support!" (env.py:750-752 -> std::runtime_error)
  4: ValueError,  # shape
  5: ValueError,  # stride
  6: ValueError,  # alignment
  7: NotImplementedError,  # unsupported feature
  8: RuntimeError,  # launch failure
  9: RuntimeError,  # no device
  10: RuntimeError,  # ABI mismatch
}

FLAG_DEBUG_SAFE_PATH = 0x1
FLAG_NO_XCD_REMAP = 0x2
FLAG_NO_BIAS_LDS = 0x8
FLAG_L2_PREFETCH = 0x10  # bench-only: touch the K/V tile two steps ahead in every prefill launch (default: the library decides; D > 512)
FLAG_NO_L2_PREFETCH = 0x20  # bench-only: never
FLAG_FORCE_SPLITS = 0x40  # bench-only: honour num_splits > 1 for prefill launches that fill the chip too
FLAG_KV_STREAM = 0x80      # bench-only: force the non-temporal K / V fetch of short-query launches
FLAG_NO_KV_STREAM = 0x800  # bench-only: never
FLAG_WIDE_TILE = 0x1000     # bench / test: prefill launches take the wide-row tile wherever one is built (default: the library decides)
FLAG_NO_WIDE_TILE = 0x2000  # bench / test: never
FLAG_PAIR_TILES = 0x8000      # bench / test: causal prefill launches pair row tiles i and n - 1 - i in one workgroup (default: the library decides)
FLAG_NO_PAIR_TILES = 0x20000  # bench / test: never
FLAG_NO_HEAD_CHUNKS = 0x80000  # bench / test: causal GQA prefill launches keep the (batch, head, row tile) workgroup order (default: the library decides; same bits either way)
FLAG_TILE_RANGES = 0x100000  # bench / test: with FLAG_FORCE_SPLITS and num_splits = n, a causal prefill launch splits every row tile's OWN visible KV tiles into n ranges
FLAG_NO_TILE_RANGES = 0x200000  # bench / test: never (default: causal launches of one round of workgroups take two)
FLAG_NO_COMPACT_GRID = 0x400000  # bench / test, packed-sequence call: keep the grid of batch x ceil(max_seqlen_q / block rows) row tiles per head (default: sized by total_q for ragged prefill batches)
FLAG_NO_PACK_GQA = 0x40000  # bench / test, packed-sequence call: decode batches under GQA keep one workgroup per QUERY head (default: a KV group's heads are the rows of one tile)
FLAG_DETERMINISTIC = 0x4000  # batch-invariant bits: no prefill KV splits, no wide-row tile, short-query splits by the KV length alone (FFPA_HIP_DETERMINISTIC=1 sets it on every call)


def FLAG_XCD_GROUP(n: int) -> int:
  """bench-only: force the number of XCDs (1, 2, 4 or 8) that share a head's row tiles (default: the library decides from the K/V footprint)"""
  return {1: 0x100, 2: 0x200, 4: 0x300, 8: 0x400}[n]

# enum ffpa_bias_dtype: additive fp16 / bf16 / fp32, or a boolean mask read as bytes (non-zero = visible)
# (torch.uint8 is NOT accepted: the public API and the reference take bool / float masks only, functional.py:860-898)
_BIAS_DTYPE = {torch.float16: 1, torch.bfloat16: 2, torch.float32: 3, torch.bool: 4}
_DTYPE = {torch.bfloat16: 0, torch.float16: 1}


class FfpaFwdParams(ctypes.Structure):
  """ctypes mirror of ``struct ffpa_fwd_params`` (include/ffpa_attn.h)."""

  _fields_ = [
    ("struct_size", ctypes.c_uint32),
    ("abi_version", ctypes.c_uint32),
    ("q", ctypes.c_void_p),
    ("k", ctypes.c_void_p),
    ("v", ctypes.c_void_p),
    ("o", ctypes.c_void_p),
    ("lse", ctypes.c_void_p),
    ("bias", ctypes.c_void_p),
    ("batch", ctypes.c_int32),
    ("heads_q", ctypes.c_int32),
    ("heads_kv", ctypes.c_int32),
    ("seqlen_q", ctypes.c_int32),
    ("seqlen_kv", ctypes.c_int32),
    ("head_dim", ctypes.c_int32),
    ("q_stride", ctypes.c_int64 * 3),
    ("k_stride", ctypes.c_int64 * 3),
    ("v_stride", ctypes.c_int64 * 3),
    ("o_stride", ctypes.c_int64 * 3),
    ("bias_stride", ctypes.c_int64 * 4),
    ("dtype", ctypes.c_int32),
    ("bias_dtype", ctypes.c_int32),
    ("causal", ctypes.c_int32),
    ("causal_offset", ctypes.c_int32),
    ("softmax_scale", ctypes.c_float),
    ("rescale_threshold", ctypes.c_float),
    ("dropout_p", ctypes.c_float),
    ("flags", ctypes.c_uint32),
    ("philox_seed", ctypes.c_uint64),
    ("philox_offset", ctypes.c_uint64),
    ("workspace", ctypes.c_void_p),
    ("workspace_bytes", ctypes.c_uint64),
    ("num_splits", ctypes.c_int32),
    ("causal_row_mod", ctypes.c_int32),
    ("kv_bounds", ctypes.c_void_p),
    ("kv_bounds_stride", ctypes.c_int64 * 2),
    ("split_tickets", ctypes.c_void_p),
  ]


class FfpaVarlenFwdParams(ctypes.Structure):
  """ctypes mirror of ``struct ffpa_varlen_fwd_params`` (include/ffpa_attn.h): the packed-sequence call."""

  _fields_ = [
    ("struct_size", ctypes.c_uint32),
    ("abi_version", ctypes.c_uint32),
    ("q", ctypes.c_void_p),
    ("k", ctypes.c_void_p),
    ("v", ctypes.c_void_p),
    ("o", ctypes.c_void_p),
    ("lse", ctypes.c_void_p),
    ("cu_seqlens_q", ctypes.c_void_p),
    ("cu_seqlens_kv", ctypes.c_void_p),
    ("seqused_kv", ctypes.c_void_p),
    ("batch", ctypes.c_int32),
    ("heads_q", ctypes.c_int32),
    ("heads_kv", ctypes.c_int32),
    ("head_dim", ctypes.c_int32),
    ("max_seqlen_q", ctypes.c_int32),
    ("max_seqlen_kv", ctypes.c_int32),
    ("q_stride", ctypes.c_int64 * 2),
    ("k_stride", ctypes.c_int64 * 2),
    ("v_stride", ctypes.c_int64 * 2),
    ("o_stride", ctypes.c_int64 * 2),
    ("lse_stride_head", ctypes.c_int64),
    ("dtype", ctypes.c_int32),
    ("causal", ctypes.c_int32),
    ("softmax_scale", ctypes.c_float),
    ("rescale_threshold", ctypes.c_float),
    ("flags", ctypes.c_uint32),
    ("reserved", ctypes.c_uint32),
    ("workspace", ctypes.c_void_p),
    ("workspace_bytes", ctypes.c_uint64),
    ("num_splits", ctypes.c_int32),
    ("total_q", ctypes.c_int32),
  ]


class FfpaPagedKv(ctypes.Structure):
  """ctypes mirror of ``struct ffpa_paged_kv`` (include/ffpa_attn.h): where the paged call's keys live."""

  _fields_ = [
    ("struct_size", ctypes.c_uint32),
    ("reserved", ctypes.c_uint32),
    ("block_table", ctypes.c_void_p),
    ("bt_stride", ctypes.c_int64),
    ("pages_per_row", ctypes.c_int32),
    ("page_size", ctypes.c_int32),
    ("num_pages", ctypes.c_int32),
    ("reserved2", ctypes.c_int32),
    ("k_page_stride", ctypes.c_int64),
    ("v_page_stride", ctypes.c_int64),
  ]


class FfpaTreeMask(ctypes.Structure):
  """ctypes mirror of ``struct ffpa_tree_mask`` (include/ffpa_attn.h): the mask words of the tree call."""

  _fields_ = [
    ("struct_size", ctypes.c_uint32),
    ("reserved", ctypes.c_uint32),
    ("bits", ctypes.c_void_p),
    ("batch_stride", ctypes.c_int64),
    ("tokens", ctypes.c_int32),
    ("reserved2", ctypes.c_int32),
  ]


class FfpaWindow(ctypes.Structure):
  """ctypes mirror of ``struct ffpa_window`` (include/ffpa_attn.h): the (left, right) of the sliding-window call."""

  _fields_ = [
    ("struct_size", ctypes.c_uint32),
    ("reserved", ctypes.c_uint32),
    ("left", ctypes.c_int32),
    ("right", ctypes.c_int32),
  ]


class FfpaMla(ctypes.Structure):
  """ctypes mirror of ``struct ffpa_mla`` (include/ffpa_attn.h): the value width and the optional append of the MLA latent-cache call."""

  _fields_ = [
    ("struct_size", ctypes.c_uint32),
    ("reserved", ctypes.c_uint32),
    ("head_dim_v", ctypes.c_int32),
    ("seqlen_new", ctypes.c_int32),
    ("kv_new", ctypes.c_void_p),
    ("cache_seqlens", ctypes.c_void_p),
    ("kv_new_stride", ctypes.c_int64 * 3),
  ]


class FfpaMlaFp8(ctypes.Structure):
  """ctypes mirror of ``struct ffpa_mla_fp8`` (include/ffpa_attn.h): the per-tensor scale of the FP8 latent-cache call."""

  _fields_ = [
    ("struct_size", ctypes.c_uint32),
    ("reserved", ctypes.c_uint32),
    ("kv_scale", ctypes.c_float),
    ("reserved2", ctypes.c_float),
  ]


class FfpaMlaSparse(ctypes.Structure):
  """ctypes mirror of ``struct ffpa_mla_sparse`` (include/ffpa_attn.h): the index list, its counts and the latent pool's geometry of the sparse latent call."""

  _fields_ = [
    ("struct_size", ctypes.c_uint32),
    ("reserved", ctypes.c_uint32),
    ("indices", ctypes.c_void_p),
    ("indices_stride", ctypes.c_int64),
    ("topk_lens", ctypes.c_void_p),
    ("kv_stride", ctypes.c_int64 * 2),
    ("topk", ctypes.c_int32),
    ("num_rows", ctypes.c_int32),
    ("head_dim_v", ctypes.c_int32),
    ("reserved2", ctypes.c_int32),
  ]


class FfpaMlaDsStoreParams(ctypes.Structure):
  """ctypes mirror of ``struct ffpa_mla_ds_store_params`` (include/ffpa_attn.h): the store of new latent rows into a pool of 656-byte FP8 rows, by slot."""

  _fields_ = [
    ("struct_size", ctypes.c_uint32),
    ("reserved", ctypes.c_uint32),
    ("kv_new", ctypes.c_void_p),
    ("slots", ctypes.c_void_p),
    ("kv_cache", ctypes.c_void_p),
    ("kv_new_stride", ctypes.c_int64 * 2),
    ("kv_cache_stride", ctypes.c_int64 * 2),
    ("tokens", ctypes.c_int32),
    ("heads_kv", ctypes.c_int32),
    ("num_rows", ctypes.c_int32),
    ("head_dim", ctypes.c_int32),
    ("dtype", ctypes.c_int32),
    ("reserved2", ctypes.c_int32),
  ]


class FfpaMlaSparseTopkParams(ctypes.Structure):
  """ctypes mirror of ``struct ffpa_mla_sparse_topk_params`` (include/ffpa_attn.h): the selection launch that makes the sparse latent calls' inputs."""

  _fields_ = [
    ("struct_size", ctypes.c_uint32),
    ("reserved", ctypes.c_uint32),
    ("scores", ctypes.c_void_p),
    ("positions", ctypes.c_void_p),
    ("cache_seqlens", ctypes.c_void_p),
    ("cu_seqlens_q", ctypes.c_void_p),
    ("block_table", ctypes.c_void_p),
    ("indices", ctypes.c_void_p),
    ("topk_lens", ctypes.c_void_p),
    ("row_stride", ctypes.c_int64),
    ("block_table_stride", ctypes.c_int64),
    ("indices_stride", ctypes.c_int64),
    ("T", ctypes.c_int32),
    ("N_or_topk", ctypes.c_int32),
    ("topk", ctypes.c_int32),
    ("B", ctypes.c_int32),
    ("W", ctypes.c_int32),
    ("page_size", ctypes.c_int32),
    ("causal", ctypes.c_int32),
    ("reserved2", ctypes.c_int32),
  ]


class FfpaMlaAppendVarlenParams(ctypes.Structure):
  """ctypes mirror of ``struct ffpa_mla_append_varlen_params`` (include/ffpa_attn.h): the latent append of a ragged step."""

  _fields_ = [
    ("struct_size", ctypes.c_uint32),
    ("reserved", ctypes.c_uint32),
    ("kv_new", ctypes.c_void_p),
    ("kv_cache", ctypes.c_void_p),
    ("cu_seqlens_q", ctypes.c_void_p),
    ("cache_seqlens", ctypes.c_void_p),
    ("seqused", ctypes.c_void_p),
    ("kv_new_stride", ctypes.c_int64 * 2),
    ("kv_cache_stride", ctypes.c_int64 * 2),
    ("batch", ctypes.c_int32),
    ("total_q", ctypes.c_int32),
    ("heads_kv", ctypes.c_int32),
    ("head_dim", ctypes.c_int32),
    ("dtype", ctypes.c_int32),
    ("reserved2", ctypes.c_int32),
  ]


class FfpaKvAppendParams(ctypes.Structure):
  """ctypes mirror of ``struct ffpa_kv_append_params`` (include/ffpa_attn.h): the KV-cache append + rotary call."""

  _fields_ = [
    ("struct_size", ctypes.c_uint32),
    ("abi_version", ctypes.c_uint32),
    ("q", ctypes.c_void_p),
    ("k", ctypes.c_void_p),
    ("v", ctypes.c_void_p),
    ("k_cache", ctypes.c_void_p),
    ("v_cache", ctypes.c_void_p),
    ("q_rot", ctypes.c_void_p),
    ("seqused", ctypes.c_void_p),
    ("cache_seqlens", ctypes.c_void_p),
    ("rotary_cos", ctypes.c_void_p),
    ("rotary_sin", ctypes.c_void_p),
    ("batch", ctypes.c_int32),
    ("heads_q", ctypes.c_int32),
    ("heads_kv", ctypes.c_int32),
    ("head_dim", ctypes.c_int32),
    ("seqlen_q", ctypes.c_int32),
    ("seqlen_new", ctypes.c_int32),
    ("capacity", ctypes.c_int32),
    ("seqlen_ro", ctypes.c_int32),
    ("q_stride", ctypes.c_int64 * 3),
    ("k_stride", ctypes.c_int64 * 3),
    ("v_stride", ctypes.c_int64 * 3),
    ("q_rot_stride", ctypes.c_int64 * 3),
    ("k_cache_stride", ctypes.c_int64 * 3),
    ("v_cache_stride", ctypes.c_int64 * 3),
    ("rotary_dim", ctypes.c_int32),
    ("rotary_interleaved", ctypes.c_int32),
    ("causal", ctypes.c_int32),
    ("dtype", ctypes.c_int32),
  ]


class FfpaKvAppendVarlenParams(ctypes.Structure):
  """ctypes mirror of ``struct ffpa_kv_append_varlen_params`` (include/ffpa_attn.h): the KV-cache append + rotary call of a ragged step."""

  _fields_ = [
    ("struct_size", ctypes.c_uint32),
    ("abi_version", ctypes.c_uint32),
    ("q", ctypes.c_void_p),
    ("k", ctypes.c_void_p),
    ("v", ctypes.c_void_p),
    ("k_cache", ctypes.c_void_p),
    ("v_cache", ctypes.c_void_p),
    ("q_rot", ctypes.c_void_p),
    ("seqused", ctypes.c_void_p),
    ("cache_seqlens", ctypes.c_void_p),
    ("cu_seqlens_q", ctypes.c_void_p),
    ("positions", ctypes.c_void_p),
    ("rotary_cos", ctypes.c_void_p),
    ("rotary_sin", ctypes.c_void_p),
    ("batch", ctypes.c_int32),
    ("heads_q", ctypes.c_int32),
    ("heads_kv", ctypes.c_int32),
    ("head_dim", ctypes.c_int32),
    ("total_q", ctypes.c_int32),
    ("capacity", ctypes.c_int32),
    ("seqlen_ro", ctypes.c_int32),
    ("rotary_dim", ctypes.c_int32),
    ("q_stride", ctypes.c_int64 * 2),
    ("k_stride", ctypes.c_int64 * 2),
    ("v_stride", ctypes.c_int64 * 2),
    ("q_rot_stride", ctypes.c_int64 * 2),
    ("k_cache_stride", ctypes.c_int64 * 3),
    ("v_cache_stride", ctypes.c_int64 * 3),
    ("rotary_interleaved", ctypes.c_int32),
    ("causal", ctypes.c_int32),
    ("dtype", ctypes.c_int32),
    ("reserved", ctypes.c_int32),
  ]


class FfpaMergeStatesParams(ctypes.Structure):
  """ctypes mirror of ``struct ffpa_merge_states_params`` (include/ffpa_attn.h): the merge of two attention states."""

  _fields_ = [
    ("struct_size", ctypes.c_uint32),
    ("abi_version", ctypes.c_uint32),
    ("o_a", ctypes.c_void_p),
    ("o_b", ctypes.c_void_p),
    ("o", ctypes.c_void_p),
    ("lse_a", ctypes.c_void_p),
    ("lse_b", ctypes.c_void_p),
    ("lse", ctypes.c_void_p),
    ("tokens", ctypes.c_int32),
    ("heads", ctypes.c_int32),
    ("head_dim", ctypes.c_int32),
    ("dtype", ctypes.c_int32),
    ("o_a_stride", ctypes.c_int64 * 2),
    ("o_b_stride", ctypes.c_int64 * 2),
    ("o_stride", ctypes.c_int64 * 2),
    ("lse_a_stride_head", ctypes.c_int64),
    ("lse_b_stride_head", ctypes.c_int64),
    ("lse_stride_head", ctypes.c_int64),
  ]


class FfpaMlaCascadePlanParams(ctypes.Structure):
  """ctypes mirror of ``struct ffpa_mla_cascade_plan_params`` (include/ffpa_attn.h): the plan launch of a shared-prefix step over the MLA latent cache."""

  _fields_ = [
    ("struct_size", ctypes.c_uint32),
    ("abi_version", ctypes.c_uint32),
    ("cu_group_seqs", ctypes.c_void_p),
    ("shared_prefix_len", ctypes.c_void_p),
    ("lens", ctypes.c_void_p),
    ("block_table", ctypes.c_void_p),
    ("cu_q_prefix", ctypes.c_void_p),
    ("prefix_lens", ctypes.c_void_p),
    ("prefix_table", ctypes.c_void_p),
    ("suffix_table", ctypes.c_void_p),
    ("suffix_lens", ctypes.c_void_p),
    ("bt_stride", ctypes.c_int64),
    ("batch", ctypes.c_int32),
    ("groups", ctypes.c_int32),
    ("pages_per_seq", ctypes.c_int32),
    ("page_size", ctypes.c_int32),
    ("seqlen_q", ctypes.c_int32),
    ("causal", ctypes.c_int32),
    ("capacity", ctypes.c_int32),
    ("shared_prefix_len_host", ctypes.c_int32),
  ]


_lib = None
_debug_lib = None
_lib_lock = threading.Lock()

_P = ctypes.POINTER
_INT, _SIZE, _VOID, _STR = ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_char_p
_VARLEN, _PAGED = [_P(FfpaVarlenFwdParams)], [_P(FfpaVarlenFwdParams), _P(FfpaPagedKv)]
_TREE = _PAGED + [_P(FfpaTreeMask)]
_WINDOW = _PAGED + [_P(FfpaWindow)]
_SOFTCAP = _WINDOW + [ctypes.c_float]
_MLA = _PAGED + [_P(FfpaMla)]
_MLA_SPARSE = [_P(FfpaVarlenFwdParams), _P(FfpaMlaSparse)]
_MLA_TREE = _MLA + [_P(FfpaTreeMask)]
_MLA_FP8 = _MLA + [_P(FfpaMlaFp8)]
_MLA_TREE_FP8 = _MLA_TREE + [_P(FfpaMlaFp8)]
_MLA_SPARSE_FP8 = _MLA_SPARSE + [_P(FfpaMlaFp8)]
# Every function include/ffpa_attn.h declares: (symbol, argtypes, restype, since).  ``since``: the ABI version that added it (0: there from the start) — the
# default library has them all; one loaded by path or through FFPA_HIP_LIBRARY (developer A/B runs load a saved build of an older commit) may lack those with
# since > 0: calling one of those is then an AttributeError.
_BINDINGS = (
  ("ffpa_attn_fwd", [_P(FfpaFwdParams), _VOID], _INT, 0),
  ("ffpa_attn_fwd_workspace_bytes", [_P(FfpaFwdParams)], _SIZE, 0),
  ("ffpa_attn_fwd_split_tickets", [_P(FfpaFwdParams)], _SIZE, 4),
  ("ffpa_attn_mask_kv_bounds", [_VOID, _INT, _P(ctypes.c_int64), _INT, _INT, _INT, _INT, _VOID, _VOID], _INT, 0),
  ("ffpa_attn_fwd_plan", [_P(FfpaFwdParams), _P(_INT)], _INT, 0),
  ("ffpa_attn_fwd_kernel", [_P(FfpaFwdParams), _STR, _SIZE], _INT, 3),
  ("ffpa_attn_varlen_fwd", _VARLEN + [_VOID], _INT, 5),
  ("ffpa_attn_varlen_fwd_plan", _VARLEN + [_P(_INT)], _INT, 5),
  ("ffpa_attn_varlen_fwd_kernel", _VARLEN + [_STR, _SIZE], _INT, 5),
  ("ffpa_attn_varlen_fwd_workspace_bytes", _VARLEN, _SIZE, 5),
  ("ffpa_attn_varlen_paged_fwd", _PAGED + [_VOID], _INT, 7),
  ("ffpa_attn_varlen_paged_fwd_plan", _PAGED + [_P(_INT)], _INT, 7),
  ("ffpa_attn_varlen_paged_fwd_kernel", _PAGED + [_STR, _SIZE], _INT, 7),
  ("ffpa_attn_varlen_paged_fwd_workspace_bytes", _PAGED, _SIZE, 7),
  ("ffpa_attn_varlen_tree_fwd", _TREE + [_VOID], _INT, 7),
  ("ffpa_attn_varlen_tree_fwd_plan", _TREE + [_P(_INT)], _INT, 7),
  ("ffpa_attn_varlen_tree_fwd_kernel", _TREE + [_STR, _SIZE], _INT, 7),
  ("ffpa_attn_varlen_tree_fwd_workspace_bytes", _TREE, _SIZE, 7),
  ("ffpa_attn_varlen_window_fwd", _WINDOW + [_VOID], _INT, 7),
  ("ffpa_attn_varlen_window_fwd_plan", _WINDOW + [_P(_INT)], _INT, 7),
  ("ffpa_attn_varlen_window_fwd_kernel", _WINDOW + [_STR, _SIZE], _INT, 7),
  ("ffpa_attn_varlen_window_fwd_workspace_bytes", _WINDOW, _SIZE, 7),
  ("ffpa_attn_varlen_softcap_fwd", _SOFTCAP + [_VOID], _INT, 7),
  ("ffpa_attn_varlen_softcap_fwd_plan", _SOFTCAP + [_P(_INT)], _INT, 7),
  ("ffpa_attn_varlen_softcap_fwd_kernel", _SOFTCAP + [_STR, _SIZE], _INT, 7),
  ("ffpa_attn_varlen_softcap_fwd_workspace_bytes", _SOFTCAP, _SIZE, 7),
  ("ffpa_attn_varlen_mla_fwd", _MLA + [_VOID], _INT, 7),
  ("ffpa_attn_varlen_mla_fwd_plan", _MLA + [_P(_INT)], _INT, 7),
  ("ffpa_attn_varlen_mla_fwd_kernel", _MLA + [_STR, _SIZE], _INT, 7),
  ("ffpa_attn_varlen_mla_fwd_workspace_bytes", _MLA, _SIZE, 7),
  ("ffpa_attn_varlen_mla_fwd_compact_slots", _MLA + [_P(_INT)], _INT, 7),
  ("ffpa_attn_varlen_mla_tree_fwd", _MLA_TREE + [_VOID], _INT, 7),
  ("ffpa_attn_varlen_mla_tree_fwd_plan", _MLA_TREE + [_P(_INT)], _INT, 7),
  ("ffpa_attn_varlen_mla_tree_fwd_kernel", _MLA_TREE + [_STR, _SIZE], _INT, 7),
  ("ffpa_attn_varlen_mla_tree_fwd_workspace_bytes", _MLA_TREE, _SIZE, 7),
  ("ffpa_attn_varlen_mla_tree_fwd_compact_slots", _MLA_TREE + [_P(_INT)], _INT, 7),
  ("ffpa_attn_mla_append_varlen", [_P(FfpaMlaAppendVarlenParams), _P(FfpaPagedKv), _VOID], _INT, 7),
  ("ffpa_attn_varlen_mla_fp8_fwd", _MLA_FP8 + [_VOID], _INT, 7),
  ("ffpa_attn_varlen_mla_fp8_fwd_plan", _MLA_FP8 + [_P(_INT)], _INT, 7),
  ("ffpa_attn_varlen_mla_fp8_fwd_kernel", _MLA_FP8 + [_STR, _SIZE], _INT, 7),
  ("ffpa_attn_varlen_mla_fp8_fwd_workspace_bytes", _MLA_FP8, _SIZE, 7),
  ("ffpa_attn_varlen_mla_fp8_fwd_compact_slots", _MLA_FP8 + [_P(_INT)], _INT, 7),
  ("ffpa_attn_mla_fp8_append_varlen", [_P(FfpaMlaAppendVarlenParams), _P(FfpaPagedKv), _P(FfpaMlaFp8), _VOID], _INT, 7),
  ("ffpa_attn_varlen_mla_sparse_fwd", _MLA_SPARSE + [_VOID], _INT, 7),
  ("ffpa_attn_varlen_mla_sparse_fwd_plan", _MLA_SPARSE + [_P(_INT)], _INT, 7),
  ("ffpa_attn_varlen_mla_sparse_fwd_kernel", _MLA_SPARSE + [_STR, _SIZE], _INT, 7),
  ("ffpa_attn_varlen_mla_sparse_fwd_workspace_bytes", _MLA_SPARSE, _SIZE, 7),
  ("ffpa_attn_varlen_mla_tree_fp8_fwd", _MLA_TREE_FP8 + [_VOID], _INT, 7),
  ("ffpa_attn_varlen_mla_tree_fp8_fwd_plan", _MLA_TREE_FP8 + [_P(_INT)], _INT, 7),
  ("ffpa_attn_varlen_mla_tree_fp8_fwd_kernel", _MLA_TREE_FP8 + [_STR, _SIZE], _INT, 7),
  ("ffpa_attn_varlen_mla_tree_fp8_fwd_workspace_bytes", _MLA_TREE_FP8, _SIZE, 7),
  ("ffpa_attn_varlen_mla_tree_fp8_fwd_compact_slots", _MLA_TREE_FP8 + [_P(_INT)], _INT, 7),
  ("ffpa_attn_varlen_mla_sparse_fp8_fwd", _MLA_SPARSE_FP8 + [_VOID], _INT, 7),
  ("ffpa_attn_varlen_mla_sparse_fp8_fwd_plan", _MLA_SPARSE_FP8 + [_P(_INT)], _INT, 7),
  ("ffpa_attn_varlen_mla_sparse_fp8_fwd_kernel", _MLA_SPARSE_FP8 + [_STR, _SIZE], _INT, 7),
  ("ffpa_attn_varlen_mla_sparse_fp8_fwd_workspace_bytes", _MLA_SPARSE_FP8, _SIZE, 7),
  ("ffpa_attn_varlen_mla_sparse_ds_fwd", _MLA_SPARSE + [_VOID], _INT, 7),
  ("ffpa_attn_varlen_mla_sparse_ds_fwd_plan", _MLA_SPARSE + [_P(_INT)], _INT, 7),
  ("ffpa_attn_varlen_mla_sparse_ds_fwd_kernel", _MLA_SPARSE + [_STR, _SIZE], _INT, 7),
  ("ffpa_attn_varlen_mla_sparse_ds_fwd_workspace_bytes", _MLA_SPARSE, _SIZE, 7),
  ("ffpa_attn_mla_ds_store", [_P(FfpaMlaDsStoreParams), _VOID], _INT, 7),
  ("ffpa_attn_mla_sparse_topk_slots", [_P(FfpaMlaSparseTopkParams), _VOID], _INT, 7),
  ("ffpa_attn_kvcache_append", [_P(FfpaKvAppendParams), _P(FfpaPagedKv), _VOID], _INT, 7),
  ("ffpa_attn_kvcache_append_varlen", [_P(FfpaKvAppendVarlenParams), _P(FfpaPagedKv), _VOID], _INT, 7),
  ("ffpa_attn_merge_states", [_P(FfpaMergeStatesParams), _VOID], _INT, 7),
  ("ffpa_attn_mla_cascade_plan", [_P(FfpaMlaCascadePlanParams), _VOID], _INT, 7),
  ("ffpa_attn_query", [_INT], _INT, 0),
  ("ffpa_attn_fwd_tile_config", [_INT, _P(_INT), _P(_INT), _P(_INT)], _INT, 0),
  ("ffpa_attn_last_error", [], _STR, 0),
  ("ffpa_attn_version", [], _STR, 0),
)
EXPORTS = tuple(b[0] for b in _BINDINGS)


def load_library(path: str | None = None) -> ctypes.CDLL:
  """dlopen the C-ABI library (after torch, so both share one HIP runtime) and bind
  every symbol ``include/ffpa_attn.h`` declares.  Raises ``RuntimeError`` if it is missing.
  """
  global _lib
  if _lib is not None and path is None:
    return _lib
  with _lib_lock:
    if _lib is not None and path is None:
      return _lib
    p = path or os.environ.get("FFPA_HIP_LIBRARY") or LIB_PATH  # (FFPA_HIP_LIBRARY: developer override — run the tests against a variant build)
    if not os.path.exists(p):
      raise RuntimeError(
        f"ffpa_attn_amd: {p} not found. The HIP extension is required (there is no fallback "
        "kernel): build it with `python -m ffpa_attn_amd.build` (needs hipcc, targets gfx950)."
      )
    lib = ctypes.CDLL(p)
    named = path is not None or p != LIB_PATH  # (a library named by the caller or by FFPA_HIP_LIBRARY: a saved build of an older commit binds what it has)
    for symbol, argtypes, restype, since in _BINDINGS:
      if named and since > 0 and not hasattr(lib, symbol):
        continue
      fn = getattr(lib, symbol)
      fn.argtypes, fn.restype = argtypes, restype
    if lib.ffpa_attn_query(0) != ABI_VERSION and path is None:
      raise RuntimeError(f"ffpa_attn_amd: {p} has ABI {lib.ffpa_attn_query(0)}, expected {ABI_VERSION}")
    if path is None:
      _lib = lib
    return lib


def load_debug_library() -> ctypes.CDLL:
  """The test-only twin of the library (``libffpa_attn_hip_test.so``: the same kernels plus the register-staged
  SAFE variants behind ``FLAG_DEBUG_SAFE_PATH``).  The product library does not carry them
  (``ffpa_attn_query(FFPA_QUERY_DEBUG_KERNELS) == 0``)."""
  global _debug_lib
  if _debug_lib is None:
    _debug_lib = load_library(TEST_LIB_PATH)
  return _debug_lib


def library_available() -> bool:
  return os.path.exists(LIB_PATH)


# Module-level capability attributes, under the names the reference's CUDA shim exports at import (``src/ffpa_attn/cuda/__init__.py:6-25``:
# read from its pybind module, ``csrc/cuffpa/ffpa_api.cc:283-305``) — call sites that gate on ``ffpa_attn.cuda.CUDA_FWD_AVAILABLE`` keep working
# against this module.  Answered lazily from ``ffpa_attn_query()`` (PEP 562: importing the package must not need the built library).  The
# reference's process-global ``set/get_cuda_backend_impl`` hint (``:38-47``, ``backend.h:16-27``) has NO equivalent on purpose: the C-ABI keeps
# no mutable global state, every choice travels in ``ffpa_fwd_params`` (SURVEY.md section 8b "Threading").
_CAPABILITY_QUERIES = {
  "HIP_FWD_AVAILABLE": 1, "CUDA_FWD_AVAILABLE": 1,  # FFPA_QUERY_FWD_AVAILABLE
  "VARLEN_FWD_AVAILABLE": 11,                        # FFPA_QUERY_VARLEN_AVAILABLE (ffpa_attn_varlen_func: the reference needs its CuTe-DSL backend for it)
  "FP16_AVAILABLE": 5, "DROPOUT_AVAILABLE": 6,       # FFPA_QUERY_FP16_AVAILABLE / _DROPOUT_AVAILABLE
}
_CAPABILITY_CONSTANTS = {
  "F16_ACC_AVAILABLE": False,        # fp32 accumulation only (the reference builds its fp16-acc kernels behind ENABLE_FFPA_F16_ACC)
  "CUDA_TMA_AVAILABLE": False,       # sm_90+ hardware feature
  "CUDA_CUTE_TMA_AVAILABLE": False,  # sm_120 CuTe kernels
  "CUDA_BWD_AVAILABLE": False,       # as in the reference: the native backend is forward-only
}


def __getattr__(name: str):
  if name == "DecodeStep":  # (the graph-replayed decode step lives above the op: ffpa_attn_amd/decode.py; reachable as hip.DecodeStep too)
    from ..decode import DecodeStep

    return DecodeStep
  if name in _CAPABILITY_CONSTANTS:
    return _CAPABILITY_CONSTANTS[name]
  if name in _CAPABILITY_QUERIES:
    try:
      return load_library().ffpa_attn_query(_CAPABILITY_QUERIES[name]) == 1
    except (RuntimeError, OSError):
      return False  # not built: the reference answers False when its extension module is missing, too
  raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


# ---- what every call of the library does, once: a stamped parameter struct, the status -> exception raise, the call on the current stream, the scratch hand-over,
# the plan read-out.  Plain functions: ``forward`` / ``varlen_forward`` run once per decoded token.
def _stamped(cls):
  """A zeroed parameter struct with its size — and, where the struct carries one (``ffpa_paged_kv`` / ``ffpa_tree_mask`` / ``ffpa_window`` / ``ffpa_mla`` ride next to a versioned struct), the ABI version — filled in."""
  p = cls()
  p.struct_size = ctypes.sizeof(cls)
  if cls not in (FfpaPagedKv, FfpaTreeMask, FfpaWindow, FfpaMla, FfpaMlaAppendVarlenParams, FfpaMlaSparse, FfpaMlaFp8, FfpaMlaDsStoreParams, FfpaMlaSparseTopkParams):
    p.abi_version = ABI_VERSION
  return p


def _raise_status(lib, rc: int, call: "str | None" = None):
  """The exception class of a non-zero ``ffpa_status`` with the library's message (``call``: the entry point, for the launches)."""
  msg = lib.ffpa_attn_last_error().decode()
  raise _STATUS_EXC.get(rc, RuntimeError)(f"{call}: {msg} (status {rc})" if call else msg)


def _call_on_stream(fn, device: torch.device, *args) -> int:
  """``fn(*args, stream)`` with ``device`` current and its current stream as the last argument."""
  with torch.cuda.device(device):
    return fn(*args, ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream))


def _deterministic_flag() -> int:
  return FLAG_DETERMINISTIC if os.environ.get("FFPA_HIP_DETERMINISTIC", "0").lower() not in ("0", "", "off", "false", "no") else 0


def _read_plan(lib, plan_fn, kernel_fn, keys: tuple, args: tuple, strict: bool = False) -> dict:
  """``{key: plan[i]}`` + ``kernel`` from a ``*_plan`` / ``*_kernel`` pair of exports; a query that fails leaves its keys out, or raises with ``strict``."""
  plan = (ctypes.c_int * len(keys))()
  rc = plan_fn(*args, plan)
  if rc != 0 and strict:
    _raise_status(lib, rc)
  out = dict(zip(keys, plan)) if rc == 0 else {}
  name = ctypes.create_string_buffer(200)
  if kernel_fn is not None and kernel_fn(*args, name, len(name)) == 0:
    out["kernel"] = name.value.decode()
  return out


_FWD_PLAN_KEYS = ("variant", "block_rows", "block_keys", "splits")
_VARLEN_PLAN_KEYS = ("row_tiles", "block_rows", "block_keys", "workgroups", "splits")


def tile_config(head_dim: int) -> dict:
  """Rows per workgroup / keys per tile / LDS bytes the kernel uses for ``head_dim``."""
  lib = load_library()
  br, bc, lds = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
  rc = lib.ffpa_attn_fwd_tile_config(int(head_dim), ctypes.byref(br), ctypes.byref(bc), ctypes.byref(lds))
  if rc != 0:
    _raise_status(lib, rc)
  return {"block_rows": br.value, "block_keys": bc.value, "lds_bytes": lds.value}


def _fwd_params(dtype: torch.dtype, batch: int, heads_q: int, heads_kv: int, seqlen_q: int, seqlen_kv: int, head_dim: int, strides, causal: bool, causal_offset: int,
                softmax_scale: float, rescale_threshold: float, dropout_p: float, flags: int, num_splits: int) -> FfpaFwdParams:
  """``ffpa_fwd_params`` without its pointers: the shape class, ``strides`` = the batch / head / row element strides of q, k, v, o, and the scalars.  The launch adds
  the tensors' addresses (bias, mask ranges, scratch, Philox state), a plan query placeholders."""
  p = _stamped(FfpaFwdParams)
  p.batch, p.heads_q, p.heads_kv = batch, heads_q, heads_kv
  p.seqlen_q, p.seqlen_kv, p.head_dim = seqlen_q, seqlen_kv, head_dim
  p.q_stride[:], p.k_stride[:], p.v_stride[:], p.o_stride[:] = strides
  p.dtype = _DTYPE[dtype]
  p.causal = 1 if causal else 0
  p.causal_offset = int(causal_offset)
  p.softmax_scale = float(softmax_scale)
  p.rescale_threshold = float(rescale_threshold)
  p.dropout_p = float(dropout_p)
  p.flags = int(flags)
  p.num_splits = int(num_splits)
  return p


def launch_plan(batch: int, heads_q: int, heads_kv: int, seqlen_q: int, seqlen_kv: int, head_dim: int, *, dtype: torch.dtype = torch.bfloat16,
                causal: bool = False, bias_dtype: "torch.dtype | None" = None, dropout_p: float = 0.0, flags: int = 0, num_splits: int = 0,
                device: "torch.device | int | None" = None, bias_row_axis: bool = True) -> dict:
  """The launch plan the library would pick for a call of this shape class — tile (``block_rows`` x ``block_keys``), KV ``splits``, ``variant``
  (0 prefill, 1 short-query) and the ``kernel`` name — without launching anything (``ffpa_attn_fwd_plan`` / ``_kernel`` on a parameter block with
  placeholder pointers; with ``device`` the plan is that GPU's: its CU count prices the split rules).  ``bias_row_axis=False``: the bias is a KEY bias
  ``[B | 1, Hq | 1, 1, Nkv]`` (row stride 0), which the builds that stage bias tiles through LDS do not serve.  A caller that cuts a batch into pieces and needs the
  pieces to run the plan of the whole (``sharding.attend_and_gather_units``) asks here."""
  lib = load_library()
  d8 = (int(head_dim) + 7) // 8 * 8
  batch, heads_q, heads_kv, seqlen_q, seqlen_kv = int(batch), int(heads_q), int(heads_kv), int(seqlen_q), int(seqlen_kv)
  strides = [(h * n * d8, n * d8, d8) for h, n in ((heads_q, seqlen_q), (heads_kv, seqlen_kv), (heads_kv, seqlen_kv), (heads_q, seqlen_q))]
  p = _fwd_params(dtype, batch, heads_q, heads_kv, seqlen_q, seqlen_kv, d8, strides, causal, seqlen_kv - seqlen_q, float(head_dim) ** -0.5, -1.0, dropout_p, flags, num_splits)
  p.q = p.k = p.v = p.o = 16
  if bias_dtype is not None:
    p.bias = 16
    p.bias_dtype = _BIAS_DTYPE[bias_dtype]
    p.bias_stride[:] = [0, 0, seqlen_kv if bias_row_axis else 0, 1]
  if num_splits != 1:
    p.workspace, p.workspace_bytes = 16, (1 << 62)
  query = (lib, lib.ffpa_attn_fwd_plan, lib.ffpa_attn_fwd_kernel, _FWD_PLAN_KEYS, (ctypes.byref(p),), True)
  if device is not None and torch.cuda.is_available():
    with torch.cuda.device(device):
      return _read_plan(*query)
  return _read_plan(*query)


def padded_head_dim(d: int) -> int:
  """The head dim of the kernel instantiation that serves ``d``: kernels are built per multiple of 64; a head dim in
  between (any multiple of 8) runs on the next one with the missing columns read as zeros and never stored — in the
  kernel, without padded copies (the reference pads on the host, csrc/cuffpa/ffpa_api.cc:123-161)."""
  return ((d + 63) // 64) * 64


def _layout_ok(t: torch.Tensor, row_dim: "int | None" = None) -> bool:
  """The layout contract of every tensor the kernels read or write through 16-byte accesses: head-dim stride 1, every other stride a (non-negative) multiple of
  8 elements, a 16-byte aligned base — and, with ``row_dim``, rows along that axis that do not overlap (split_d.cuh:137-142 assumed dense [B,H,N,D]; here
  arbitrary batch / head / row strides are honoured)."""
  ok = t.stride(-1) == 1 and all(s % 8 == 0 and s >= 0 for s in t.stride()[:-1]) and t.data_ptr() % 16 == 0
  if ok and row_dim is not None and t.size(row_dim) > 1 and t.stride(row_dim) < t.size(-1):
    ok = False  # overlapping rows
  return ok


def _rows(t: torch.Tensor, row_dim: "int | None" = None) -> torch.Tensor:
  """``t`` if it satisfies the layout contract, else a dense copy (only pathological views are copied)."""
  if t.is_contiguous():
    return t  # (a dense tensor is its own dense copy: nothing to decide, and the decode path's tensors are dense)
  return t if _layout_ok(t, row_dim) else t.contiguous()


def _pad_head_dim(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor):
  """Rows must be whole 16-byte slots: only a head dim that is not a multiple of 8 is padded (copies) -> ``(q, k, v, padded head dim)``; the call slices its
  output back with ``_unpad_head_dim``."""
  D = q.size(-1)
  Dp = (D + 7) // 8 * 8
  if Dp != D:
    pad = (0, Dp - D)
    q, k, v = (torch.nn.functional.pad(t, pad) for t in (q, k, v))
  return q, k, v, Dp


def _unpad_head_dim(o: torch.Tensor, D: int) -> torch.Tensor:
  return o[..., :D].contiguous() if o.size(-1) != D else o  # the ops' contract (and their fake impls): a dense tensor of the caller's head dim


def mask_kv_bounds(attn_bias: torch.Tensor, nq: int, nkv: int) -> torch.Tensor:
  """Key ranges of an additive (-inf = hidden, 0 = neutral) or boolean (False = hidden) mask for the kernel's tile clipping:
  int32 ``[Bb, Hb, ceil(Nq/32), 4]`` holding, per block of 32 query rows, ``[first, end)`` such that every key outside is
  hidden for every row of the block (``{Nkv, 0}`` for a block without any visible key) and ``[free_first, free_end)``, the
  first run of keys on which the mask does nothing for every row of the block (``{0, 0}``: none) — tiles inside it are
  computed without reading the mask.  On the GPU: one fused pass of the library over the mask
  (``ffpa_attn_mask_kv_bounds``); elsewhere (tests) the same thing in torch ops."""
  bb, hb = attn_bias.size(0), attn_bias.size(1)
  nblk = (nq + 31) // 32
  if attn_bias.is_cuda and attn_bias.dtype in _BIAS_DTYPE:
    lib = load_library()
    out = torch.empty((bb, hb, nblk, 4), dtype=torch.int32, device=attn_bias.device)
    strides = (ctypes.c_int64 * 4)(*[attn_bias.stride(d) if attn_bias.size(d) > 1 else 0 for d in range(4)])
    rc = _call_on_stream(lib.ffpa_attn_mask_kv_bounds, attn_bias.device, ctypes.c_void_p(attn_bias.data_ptr()), _BIAS_DTYPE[attn_bias.dtype], strides, bb, hb, nq, nkv,
                         ctypes.c_void_p(out.data_ptr()))
    if rc != 0:
      _raise_status(lib, rc)
    return out
  is_bool = attn_bias.dtype in (torch.bool, torch.uint8)
  vis = attn_bias.ne(0) if is_bool else ~torch.isneginf(attn_bias)      # [Bb, Hb, Nq|1, Nkv|1]
  neutral = attn_bias.ne(0) if is_bool else attn_bias.eq(0)
  pad = nblk * 32 - nq

  def per_block(t, pad_value, reduce):
    t = t.expand(bb, hb, nq, nkv)
    if pad:
      t = torch.nn.functional.pad(t, (0, 0, 0, pad), value=pad_value)  # rows past Nq: see nothing / constrain nothing
    t = t.reshape(bb, hb, nblk, 32, nkv)
    return t.any(dim=3) if reduce == "any" else t.all(dim=3)            # [Bb, Hb, nblk, Nkv]

  col_any, col_all = per_block(vis, False, "any"), per_block(neutral, True, "all")
  idx = torch.arange(nkv, device=attn_bias.device, dtype=torch.int32)
  first = torch.where(col_any, idx, torch.full_like(idx, nkv)).amin(dim=-1)
  end = torch.where(col_any, idx + 1, torch.zeros_like(idx)).amax(dim=-1)
  ff = torch.where(col_all, idx, torch.full_like(idx, nkv)).amin(dim=-1)                           # first neutral key
  after = (~col_all) & (idx >= ff.unsqueeze(-1))
  fe = torch.where(after, idx, torch.full_like(idx, nkv)).amin(dim=-1)                              # first non-neutral key after it
  none = ff >= nkv
  ff, fe = torch.where(none, torch.zeros_like(ff), ff), torch.where(none, torch.zeros_like(fe), fe)
  return torch.stack((first, end, ff, fe), dim=-1).to(torch.int32).contiguous()


# One scan per mask instead of one per call — OPT-IN (FFPA_HIP_MASK_BOUNDS_CACHE=1): a static mask (the same causal / padding /
# sliding-window tensor for every layer and step) is then scanned once.  An entry is valid only while the very tensor object it was
# computed from (the view's base: the public API re-views the caller's mask on every call) is still alive — so its memory cannot have
# been recycled for another mask — and torch's in-place version counter (shared by all views of a storage, bumped by every in-place
# write torch knows of) has not moved.  What the counter does NOT see leaves stale ranges behind, and stale ranges make the kernel skip
# visible keys silently: `mask.data.fill_()`, a Triton / custom kernel writing through the raw pointer, a graph replay refreshing a
# static mask buffer.  Hence off unless the caller asks for it and knows its masks are written through torch ops only.  Tensors
# without a version counter (created under torch.inference_mode()) are never cached.  An entry remembers the stream its scan ran
# on and an event behind it: a consumer on another stream waits for that event first.  Holds the small int32 result only.
_BOUNDS_CACHE: "dict[tuple, tuple]" = {}
_BOUNDS_CACHE_MAX = 16


def _mask_bounds_cache_enabled() -> bool:
  return os.environ.get("FFPA_HIP_MASK_BOUNDS_CACHE", "0") not in ("0", "")


def _tensor_version(t: torch.Tensor):
  """torch's in-place version counter of ``t``, or None for tensors that do not track one (inference tensors raise on access)."""
  try:
    if t.is_inference():
      return None
    return t._version
  except RuntimeError:
    return None


def cached_mask_kv_bounds(attn_bias: torch.Tensor, nq: int, nkv: int) -> torch.Tensor:
  import weakref

  version = _tensor_version(attn_bias)
  if version is None:  # no version counter: nothing would ever invalidate the entry
    return mask_kv_bounds(attn_bias, nq, nkv)
  owner = attn_bias._base if attn_bias._base is not None else attn_bias
  key = (id(owner), attn_bias.data_ptr(), attn_bias.dtype, tuple(attn_bias.shape), tuple(attn_bias.stride()), nq, nkv)
  stream = torch.cuda.current_stream(attn_bias.device)
  hit = _BOUNDS_CACHE.get(key)
  if hit is not None:
    ref, ver, out, src_stream, event = hit
    if ref() is owner and ver == version:
      if src_stream != stream.cuda_stream:
        stream.wait_event(event)  # the scan ran on another stream: order this stream's launch behind it
      return out
  out = mask_kv_bounds(attn_bias, nq, nkv)
  event = torch.cuda.Event()
  event.record(stream)
  for k_ in [k_ for k_, ent in _BOUNDS_CACHE.items() if ent[0]() is None]:  # owners that died
    del _BOUNDS_CACHE[k_]
  if len(_BOUNDS_CACHE) >= _BOUNDS_CACHE_MAX:
    _BOUNDS_CACHE.pop(next(iter(_BOUNDS_CACHE)))
  _BOUNDS_CACHE[key] = (weakref.ref(owner), version, out, stream.cuda_stream, event)
  return out


def _want_mask_bounds(attn_bias: torch.Tensor, b: int, hq: int, nq: int, nkv: int) -> bool:
  """The scan reads the mask once (2-4 B per element): worth it for every mask that has real row and key axes and a
  problem with tiles to skip, unless each (batch, head) pair brings its own mask (then the scan is as big as the
  mask reads of the attention itself).  FFPA_HIP_MASK_BOUNDS=0/1 forces it off / on."""
  env = os.environ.get("FFPA_HIP_MASK_BOUNDS")
  if env is not None:
    return env not in ("0", "")
  if attn_bias.size(2) != nq or attn_bias.size(3) != nkv or nkv < 512 or nq < 128:
    return False
  return b * hq >= 2 * attn_bias.size(0) * attn_bias.size(1)


# Per-(device, stream) scratch of the KV-split launches.  Launches on one stream are ordered, so they may share a buffer; launches on different
# streams may overlap and get their own.  Both tables are small LRU maps (a process that churns through streams does not accumulate buffers).
#   _TICKETS:    zeroed int32 counters for the in-launch merge (ffpa_fwd_params.split_tickets): zeroed once — the kernel leaves every counter at
#                zero — and grown on demand;
#   _WORKSPACES: the fp32 partials + LSE of the short-query (decode) launches — a fresh torch.empty per token was a fifth of the host time of a
#                decode step.  Only workspaces up to _WORKSPACE_KEEP_BYTES are kept; the transient hundreds of MiB of a split PREFILL launch go
#                back to the caching allocator as before.
_SCRATCH_MAX_STREAMS = 32
_WORKSPACE_KEEP_BYTES = 8 << 20
_TICKETS: "dict[tuple, torch.Tensor]" = {}
_WORKSPACES: "dict[tuple, torch.Tensor]" = {}


def _lru_get(table: dict, key):
  t = table.pop(key, None)
  if t is not None:
    table[key] = t  # (re-inserted: dicts keep insertion order, the first key is the least recently used)
  return t


def _lru_put(table: dict, key, value) -> None:
  table.pop(key, None)
  while len(table) >= _SCRATCH_MAX_STREAMS:
    table.pop(next(iter(table)))
  table[key] = value


def _split_tickets(device: torch.device, stream: int, n: int) -> torch.Tensor:
  if torch.cuda.is_current_stream_capturing():
    # inside a stream capture: a buffer of the graph's own pool, zeroed by a node of the graph (like the workspace, it is replayed in place)
    return torch.zeros(n, dtype=torch.int32, device=device)
  key = (device.index, stream)
  t = _lru_get(_TICKETS, key)
  if t is None or t.numel() < n:
    t = torch.zeros(max(4096, n), dtype=torch.int32, device=device)
    _lru_put(_TICKETS, key, t)
  return t


def _workspace(device: torch.device, stream: int, nbytes: int) -> torch.Tensor:
  words = (nbytes + 3) // 4
  if nbytes > _WORKSPACE_KEEP_BYTES or torch.cuda.is_current_stream_capturing():
    return torch.empty(words, dtype=torch.float32, device=device)  # caching allocator (under capture: the graph's pool, replayed in place)
  key = (device.index, stream)
  t = _lru_get(_WORKSPACES, key)
  if t is None or t.numel() < words:
    t = torch.empty(max(words, 1 << 16), dtype=torch.float32, device=device)
    _lru_put(_WORKSPACES, key, t)
  return t


def _hand_over_workspace(p, device: torch.device, stream: int, nbytes: int) -> "torch.Tensor | None":
  """Point ``p.workspace`` at ``nbytes`` of this stream's scratch; the caller holds the returned tensor in a local until its launch has been enqueued."""
  if not nbytes:
    return None
  workspace = _workspace(device, stream, nbytes)
  p.workspace = workspace.data_ptr()
  p.workspace_bytes = nbytes
  return workspace


# What a launch needs besides its tensors — workspace bytes and ticket count — is a function of the shape class only (ffpa_capi.hip make_plan): asked
# once per class, not once per call (two ctypes round trips less per decode token).  The class names everything make_plan prices with (the mask KIND too: the
# wide-row tile of D = 320 is for boolean masks only, and another tile is another number of workgroups); the library clamps the split count to the scratch it is
# handed, so a class missing from the key could cost splits, never memory safety.
_PLAN_SCRATCH: "dict[tuple, tuple[int, int]]" = {}


def _cached_scratch(table: dict, key: tuple, ask):
  """``table[key]``, or — the first call of a shape class — what ``ask()`` gets from the library; a table of 512 classes starts over."""
  hit = table.get(key)
  if hit is None:
    if len(table) >= 512:
      table.clear()
    hit = table[key] = ask()
  return hit


def _plan_scratch(lib, p: "FfpaFwdParams", num_splits: int, want_tickets: bool, device_index: int) -> tuple[int, int]:
  if num_splits == 1:
    return 0, 0
  key = (id(lib), device_index, p.dtype, p.batch, p.heads_q, p.heads_kv, p.seqlen_q, p.seqlen_kv, p.head_dim, p.causal, p.bias_dtype if p.bias else 0,
         bool(p.bias) and p.bias_stride[2] == 0, p.kv_bounds is not None, p.dropout_p > 0.0, p.flags, num_splits, p.causal_row_mod, p.causal_offset, want_tickets, os.environ.get("FFPA_HIP_FAKE_CUS"))

  def ask():
    ws = int(lib.ffpa_attn_fwd_workspace_bytes(ctypes.byref(p)))
    nt = int(lib.ffpa_attn_fwd_split_tickets(ctypes.byref(p))) if (ws and want_tickets and hasattr(lib, "ffpa_attn_fwd_split_tickets")) else 0
    return ws, nt

  return _cached_scratch(_PLAN_SCRATCH, key, ask)


def forward(
  q: torch.Tensor,
  k: torch.Tensor,
  v: torch.Tensor,
  attn_bias: torch.Tensor | None,
  causal: bool,
  softmax_scale: float,
  *,
  causal_offset: int | None = None,
  rescale_threshold: float = -1.0,
  dropout_p: float = 0.0,
  philox_seed: int = 0,
  philox_offset: int = 0,
  flags: int = 0,
  return_lse: bool = True,
  num_splits: int = 0,
  plan_out: dict | None = None,
  kv_bounds: torch.Tensor | bool | None = None,
  causal_row_mod: int = 0,
  merge_in_launch: bool | None = None,
) -> tuple[torch.Tensor, torch.Tensor | None]:
  """Run the gfx950 kernel on the current stream of ``q.device``; returns ``(o, lse)``.

  Inputs are ``[B, H, N, D]`` bf16/fp16 device tensors.  ``causal_offset=None`` selects the
  reference's tail-aligned causal mask (``Nkv - Nq``, split_d.cuh:222-228).

  Short-query calls (the reference's decode regime, ``Nq`` in 1..7 reaches FFPA: functional.py:722-723):
  with GQA and no bias, the ``group`` query heads of a KV head are packed into the row axis
  (``q`` viewed as ``[B, Hkv, group*Nq, D]`` — K/V are then streamed once per KV head instead of once
  per query head), the library splits the KV axis over workgroups (``num_splits``: 0 = heuristic,
  1 = never) and merges by LSE; the scratch for the partials is allocated here with torch.
  ``plan_out``, if given, receives the launch plan (variant, block_rows, block_keys, splits, packed).

  ``merge_in_launch``: short-query KV-split launches merge their partials inside the launch (the last split of a row tile to arrive does
  it: one launch per call) instead of launching the merge kernel behind the split kernel — the same numbers.  OFF by default
  (``FFPA_HIP_MERGE_IN_LAUNCH=1`` or ``True`` turns it on): measured on MI355X the hand-off costs every split workgroup more than
  the second launch costs the call (decode B1 H32 Nkv 8192 D512: 115 vs 110 us; profiles/r03_split_merge.txt).

  ``kv_bounds``: key ranges of the mask (``mask_kv_bounds``) — the kernel then skips the KV tiles the mask hides
  entirely and does not read the mask for the tiles it leaves untouched (an explicit causal mask costs what ``is_causal``
  costs); ``None`` derives them from ``attn_bias``
  when that is worth a scan of the mask, ``False`` never, ``True`` always, or pass a precomputed tensor.  The scan runs on
  every call; ``FFPA_HIP_MASK_BOUNDS_CACHE=1`` keeps the ranges per (mask tensor, torch version counter) instead — only safe when
  the mask is written through torch ops alone (``mask.data`` writes, raw-pointer kernels and graph replays do not move the counter and
  would leave stale ranges, i.e. silently skipped keys); masks created under ``torch.inference_mode()`` are never cached.
  """
  if not q.is_cuda:
    raise NotImplementedError(
      f"ffpa_attn::_fwd_hip has no implementation for device '{q.device.type}' (the HIP kernel needs a GPU tensor)"
    )
  lib = load_debug_library() if (flags & FLAG_DEBUG_SAFE_PATH) else load_library()
  if q.dtype not in _DTYPE or k.dtype != q.dtype or v.dtype != q.dtype:
    raise TypeError(f"ffpa_attn::_fwd_hip only supports fp16/bf16 q/k/v of one dtype, got {q.dtype}, {k.dtype}, {v.dtype}")
  # The kernel takes raw pointers: everything its buffer descriptors assume is checked here, as the reference's
  # launcher does with TORCH_CHECK (csrc/cuffpa/launch.cuh:79-129) — the public API validates earlier, but the
  # registered op can be called directly.
  if q.dim() != 4 or k.dim() != 4 or v.dim() != 4:
    raise ValueError("ffpa_attn::_fwd_hip: q/k/v must be 4-D [B, H, N, D] tensors")
  if k.shape != v.shape:
    raise ValueError(f"ffpa_attn::_fwd_hip: key and value must have the same shape, got {tuple(k.shape)} and {tuple(v.shape)}")
  if k.size(0) != q.size(0) or k.size(3) != q.size(3):
    raise ValueError(f"ffpa_attn::_fwd_hip: q {tuple(q.shape)} and k/v {tuple(k.shape)} must share batch size and head dim")
  if k.size(1) == 0 or q.size(1) % k.size(1) != 0:
    raise ValueError(f"ffpa_attn::_fwd_hip: query num_heads ({q.size(1)}) must be a multiple of key/value num_heads ({k.size(1)})")
  if k.device != q.device or v.device != q.device:
    raise ValueError(f"ffpa_attn::_fwd_hip: q/k/v must be on one device, got {q.device}, {k.device}, {v.device}")
  if attn_bias is not None and attn_bias.numel() > 0 and attn_bias.device != q.device:
    raise ValueError(f"ffpa_attn::_fwd_hip: attn_bias must be on q's device, got {attn_bias.device} and {q.device}")
  B, Hq, Nq, D = q.shape
  _, Hkv, Nkv, _ = k.shape
  out_shape = (B, Hq, Nq)
  if causal_offset is None:
    causal_offset = Nkv - Nq
  q, k, v, Dp = _pad_head_dim(q, k, v)
  group = Hq // Hkv if Hkv and Hq % Hkv == 0 else 1
  has_bias = attn_bias is not None and attn_bias.numel() > 0
  packed = causal_row_mod == 0 and group > 1 and Nq <= 7 and group * Nq <= 32 and not has_bias and dropout_p == 0.0
  if packed:
    # [B, Hq, Nq, D] -> [B, Hkv, group*Nq, D]: packed row r = (head in group) * Nq + (query row)
    q = q.contiguous().view(B, Hkv, group * Nq, Dp)
    causal_row_mod = Nq
    Hq, Nq = Hkv, group * Nq
  q, k, v = _rows(q, 2), _rows(k, 2), _rows(v, 2)
  o = torch.empty((B, Hq, Nq, Dp), dtype=q.dtype, device=q.device)
  lse = torch.empty((B, Hq, Nq), dtype=torch.float32, device=q.device) if return_lse else None
  if num_splits == 0 and Nq > 32 and os.environ.get("FFPA_HIP_PREFILL_SPLITS", "1").lower() in ("0", "off", "false", "no"):
    # opt-out of the KV-split rules for PREFILL launches (under-filled / part of a round / ragged round: ffpa_capi.hip make_plan): they allocate fp32
    # scratch of splits x B x Hq x Nq x (D + 1) x 4 bytes per call (up to kMaxAutoWorkspaceBytes = 1 GiB) and make the bits of a (batch, head) slice depend on
    # how many heads share the launch (fp32 partials + LSE merge: equal to rounding, not to the bit).  Short-query (decode) launches keep their rule.
    num_splits = 1

  p = _fwd_params(q.dtype, B, Hq, Hkv, Nq, Nkv, Dp, [t.stride()[:3] for t in (q, k, v, o)], causal, causal_offset, softmax_scale, rescale_threshold, dropout_p,
                  int(flags) | _deterministic_flag(), num_splits)
  p.q, p.k, p.v, p.o = q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr()
  p.lse = lse.data_ptr() if lse is not None else None
  if attn_bias is not None and attn_bias.numel() > 0:
    if attn_bias.dim() != 4:
      raise ValueError("attn_bias must be 4-D [B|1, Hq|1, Nq|1, Nkv|1]")
    if attn_bias.dtype not in _BIAS_DTYPE:
      raise TypeError(f"attn_bias dtype must be fp16/bf16/fp32 (additive) or bool (mask), got {attn_bias.dtype}")
    full = (B, Hq, Nq, Nkv)
    strides = []
    for dim in range(4):
      if attn_bias.size(dim) == full[dim]:
        strides.append(attn_bias.stride(dim) if full[dim] > 1 else 0)
      elif attn_bias.size(dim) == 1:
        strides.append(0)  # broadcast dims use stride 0 (native/launch.cuh:277-290)
      else:
        raise ValueError(f"attn_bias dim {dim} must be 1 or {full[dim]}, got {attn_bias.size(dim)}")
    p.bias = attn_bias.data_ptr()
    p.bias_dtype = _BIAS_DTYPE[attn_bias.dtype]
    p.bias_stride[:] = strides
    if kv_bounds is True or (kv_bounds is None and _want_mask_bounds(attn_bias, B, Hq, Nq, Nkv)):
      # (the scan is skipped under stream capture / compile tracing only in the sense that the cache is not consulted there: a
      # captured graph must contain the scan kernel it depends on)
      capturing = torch.cuda.is_current_stream_capturing()
      kv_bounds = cached_mask_kv_bounds(attn_bias, Nq, Nkv) if (_mask_bounds_cache_enabled() and not capturing) else mask_kv_bounds(attn_bias, Nq, Nkv)
    if isinstance(kv_bounds, torch.Tensor):
      nblk = (Nq + 31) // 32
      if kv_bounds.dtype != torch.int32 or kv_bounds.dim() != 4 or kv_bounds.shape[2:] != (nblk, 4) or not kv_bounds.is_contiguous():
        raise ValueError(f"kv_bounds must be a contiguous int32 [B|1, Hq|1, {nblk}, 4] tensor (mask_kv_bounds)")
      if kv_bounds.size(0) not in (1, B) or kv_bounds.size(1) not in (1, Hq) or kv_bounds.device != q.device:
        raise ValueError("kv_bounds batch / head dims must be 1 or match q, on q's device")
      p.kv_bounds = kv_bounds.data_ptr()
      p.kv_bounds_stride[:] = [kv_bounds.stride(0) if kv_bounds.size(0) > 1 else 0, kv_bounds.stride(1) if kv_bounds.size(1) > 1 else 0]
  p.causal_row_mod = int(causal_row_mod)
  p.philox_seed = int(philox_seed) & 0xFFFFFFFFFFFFFFFF
  p.philox_offset = int(philox_offset) & 0xFFFFFFFFFFFFFFFF

  tickets = None
  with torch.cuda.device(q.device):
    stream = torch.cuda.current_stream(q.device).cuda_stream
    if merge_in_launch is None:
      merge_in_launch = os.environ.get("FFPA_HIP_MERGE_IN_LAUNCH", "0") not in ("0", "")
    ws_bytes, n_tickets = _plan_scratch(lib, p, num_splits, bool(merge_in_launch), q.device.index or 0)
    workspace = _hand_over_workspace(p, q.device, stream, ws_bytes)  # (held in a local until the launch below has been enqueued)
    if workspace is not None and n_tickets:
      tickets = _split_tickets(q.device, stream, n_tickets)
      p.split_tickets = tickets.data_ptr()
    if plan_out is not None:
      plan = _read_plan(lib, lib.ffpa_attn_fwd_plan, getattr(lib, "ffpa_attn_fwd_kernel", None), _FWD_PLAN_KEYS, (ctypes.byref(p),))
      if "variant" in plan:
        plan["packed"] = bool(packed)
      plan_out.update(plan)
    rc = lib.ffpa_attn_fwd(ctypes.byref(p), ctypes.c_void_p(stream))
  if rc != 0:
    if tickets is not None:
      tickets.zero_()  # a launch that did not complete may have left counters behind: the next call must start from zeros
    _raise_status(lib, rc, "ffpa_attn_fwd")
  del tickets
  if packed:
    o = o.view(*out_shape, Dp)
    lse = lse.view(out_shape) if lse is not None else None
  return _unpad_head_dim(o, D), lse


# ----------------------------------------------------------------------------------
# torch.library op.  Same leading schema as ffpa_attn::_fwd_cuda
# (src/ffpa_attn/cuda/__init__.py:57-66); the fp8/fp4 tail of that schema is dropped
# (bf16/fp16 only) and two trailing knobs are added with defaults.
# ----------------------------------------------------------------------------------
_OP_NAMESPACE = "ffpa_attn"

torch.library.define(
  f"{_OP_NAMESPACE}::_fwd_hip",
  "(Tensor q, Tensor k, Tensor v, Tensor attn_bias, int stages, int acc, int causal, "
  "float softmax_scale, float dropout_p, int philox_seed, int philox_offset, "
  "int causal_offset=-2147483648, float rescale_threshold=-1.0, Tensor? kv_bounds=None) -> (Tensor o, Tensor softmax_lse)",
)

_AUTO_OFFSET = -2147483648


@torch.library.impl(f"{_OP_NAMESPACE}::_fwd_hip", "CUDA")  # ROCm tensors dispatch on the CUDA key
def _fwd_hip_torch_op(
  q,
  k,
  v,
  attn_bias,
  stages,
  acc,
  causal,
  softmax_scale,
  dropout_p,
  philox_seed,
  philox_offset,
  causal_offset=_AUTO_OFFSET,
  rescale_threshold=-1.0,
  kv_bounds=None,
):
  del stages, acc  # tile/pipeline shape is fixed per head dim; accumulation is always fp32
  o, lse = forward(
    q,
    k,
    v,
    attn_bias if attn_bias.numel() > 0 else None,
    bool(causal),
    softmax_scale,
    causal_offset=None if causal_offset == _AUTO_OFFSET else causal_offset,
    rescale_threshold=rescale_threshold,
    dropout_p=dropout_p,
    philox_seed=philox_seed,
    philox_offset=philox_offset,
    kv_bounds=kv_bounds,
  )
  return o, lse


@torch.library.register_fake(f"{_OP_NAMESPACE}::_fwd_hip")
def _fwd_hip_fake(
  q,
  k,
  v,
  attn_bias,
  stages,
  acc,
  causal,
  softmax_scale,
  dropout_p,
  philox_seed,
  philox_offset,
  causal_offset=_AUTO_OFFSET,
  rescale_threshold=-1.0,
  kv_bounds=None,
):
  B, Hq, Nq, D = q.shape
  o = q.new_empty((B, Hq, Nq, D))
  lse = q.new_empty((B, Hq, Nq), dtype=torch.float32)
  return o, lse


def ffpa_attn_forward_hip(
  q: torch.Tensor,
  k: torch.Tensor,
  v: torch.Tensor,
  attn_bias: torch.Tensor | None,
  *,
  causal: bool,
  softmax_scale: float,
  dropout_p: float = 0.0,
  philox_seed: int = 0,
  philox_offset: int = 0,
  causal_offset: int | None = None,
  rescale_threshold: float = -1.0,
  kv_bounds: torch.Tensor | None = None,
) -> tuple[torch.Tensor, torch.Tensor]:
  """Python-level entry (the analogue of ``_ffpa_attn_forward_cuda``, cuda/_ffpa_fwd.py:6-62):
  converts ``attn_bias=None`` into the empty tensor the op schema expects and calls the op.  ``kv_bounds``: precomputed key ranges of
  the mask (``mask_kv_bounds``), ``None`` = derived per call."""
  if attn_bias is None:
    attn_bias = q.new_empty((0,))
  return torch.ops.ffpa_attn._fwd_hip(
    q,
    k,
    v,
    attn_bias,
    0,
    1,
    int(causal),
    float(softmax_scale),
    float(dropout_p),
    int(philox_seed),
    int(philox_offset),
    _AUTO_OFFSET if causal_offset is None else int(causal_offset),
    float(rescale_threshold),
    kv_bounds,
  )


# ----------------------------------------------------------------------------------
# Packed sequences (ffpa_attn_varlen_func): the launch wrapper and its torch.library op.  Replaces the reference's
# ffpa_attn::_varlen_fwd_cute (src/ffpa_attn/cute/__init__.py:792-880), which only its CuTe-DSL backend serves.
# ----------------------------------------------------------------------------------
def _varlen_params(dtype: torch.dtype, batch: int, heads_q: int, heads_kv: int, head_dim: int, max_seqlen_q: int, max_seqlen_k: int, total_q: int, strides, causal: bool,
                   softmax_scale: float, rescale_threshold: float, flags: int, num_splits: int) -> FfpaVarlenFwdParams:
  """``ffpa_varlen_fwd_params`` without its pointers: the shape class, ``strides`` = the row / head element strides of q, k, v, o, and the scalars.  The launch adds
  the tensors' addresses (and its scratch), a plan query placeholders."""
  p = _stamped(FfpaVarlenFwdParams)
  p.batch, p.heads_q, p.heads_kv, p.head_dim = batch, heads_q, heads_kv, head_dim
  p.max_seqlen_q, p.max_seqlen_kv = int(max_seqlen_q), int(max_seqlen_k)
  p.q_stride[:], p.k_stride[:], p.v_stride[:], p.o_stride[:] = strides
  p.dtype = _DTYPE[dtype]
  p.causal = 1 if causal else 0
  p.softmax_scale = float(softmax_scale)
  p.rescale_threshold = float(rescale_threshold)
  p.flags = int(flags)
  p.num_splits = int(num_splits)
  p.total_q = total_q
  return p


def _paged_kv(block_table: int, bt_stride: int, pages_per_row: int, page_size: int, num_pages: int, k_page_stride: int, v_page_stride: int) -> FfpaPagedKv:
  """``ffpa_paged_kv``: the block table's address and row stride, the pool's geometry and its K / V page strides (elements)."""
  kv = _stamped(FfpaPagedKv)
  kv.block_table, kv.bt_stride, kv.pages_per_row = block_table, bt_stride, pages_per_row
  kv.page_size, kv.num_pages = page_size, num_pages
  kv.k_page_stride, kv.v_page_stride = k_page_stride, v_page_stride
  return kv


def _paged_kv_of(block_table: torch.Tensor, k: torch.Tensor, v: torch.Tensor) -> "tuple[FfpaPagedKv, torch.Tensor]":
  """``ffpa_paged_kv`` of a block table ``[B, pages_per_row]`` over the pools ``k`` / ``v [num_pages, page_size, Hkv, D]`` -> ``(kv, the table it points at)``: a table whose
  rows are not dense is copied, and the caller keeps that copy alive until its launch has been enqueued."""
  if block_table.stride(1) != 1 or block_table.data_ptr() % 4 != 0:
    block_table = block_table.contiguous()
  return _paged_kv(block_table.data_ptr(), block_table.stride(0), block_table.size(1), k.size(1), k.size(0), k.stride(0), v.stride(0)), block_table


# The call families over a K and a V cache and their launch exports (the tree, window and soft-capping calls serve both caches: their ``kv`` may be NULL)
_VARLEN_EXPORTS = {"packed": "ffpa_attn_varlen_fwd", "paged": "ffpa_attn_varlen_paged_fwd", "tree": "ffpa_attn_varlen_tree_fwd",
                   "window": "ffpa_attn_varlen_window_fwd", "softcap": "ffpa_attn_varlen_softcap_fwd"}


def _varlen_fn(lib, family: str, suffix: str = ""):
  """The export of a family of ``_VARLEN_EXPORTS`` with this suffix ("" the launch, "_plan", "_kernel", "_workspace_bytes")"""
  return getattr(lib, _VARLEN_EXPORTS[family] + suffix)


# Scratch of a KV-split packed launch: a function of the shape class (ffpa_capi.hip varlen_plan), asked once per class
_VARLEN_SCRATCH: "dict[tuple, int]" = {}


def _varlen_scratch(lib, p: "FfpaVarlenFwdParams", device_index: int, family: str, paged: bool, args: tuple, window: "tuple | None" = None) -> int:
  if p.num_splits == 1 or p.flags & FLAG_DETERMINISTIC:
    return 0
  key = (id(lib), device_index, p.dtype, p.batch, p.heads_q, p.heads_kv, p.head_dim, p.max_seqlen_q, p.max_seqlen_kv, p.total_q, p.causal, p.flags, p.num_splits, os.environ.get("FFPA_HIP_FAKE_CUS"),
         paged, {"tree": True, "window": "window", "softcap": "softcap"}.get(family, False), window)  # (the key's values are the ones it has always held)
  return _cached_scratch(_VARLEN_SCRATCH, key, lambda: int(_varlen_fn(lib, family, "_workspace_bytes")(*args)))


def varlen_forward(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, cu_seqlens_q: torch.Tensor, cu_seqlens_k: "torch.Tensor | None", max_seqlen_q: int,
                   max_seqlen_k: int, causal: bool, softmax_scale: float, *, rescale_threshold: float = -1.0, return_lse: bool = True, flags: int = 0,
                   plan_out: "dict | None" = None, seqused_k: "torch.Tensor | None" = None, num_splits: int = 0, block_table: "torch.Tensor | None" = None,
                   tree_words: "torch.Tensor | None" = None, window: "tuple[int, int] | None" = None, softcap: float = 0.0):
  """One launch of the packed-sequence kernel: ``q [T_q, Hq, D]``, ``k`` / ``v [T_k, Hkv, D]``, int32 device ``cu_seqlens_*`` ``[B + 1]`` ->
  ``(o [T_q, Hq, D], lse [Hq, T_q] fp32 | None)``.  Nothing is read back to the host and nothing synchronises: the call captures into a HIP graph.
  Rows without a visible key: O = 0, LSE = -inf.

  ``seqused_k`` (int32 device ``[B]``, this build's extension at the op level — the public ``ffpa_attn_varlen_func`` rejects it like the reference's): sequence i
  uses only the first ``seqused_k[i]`` of its key rows — a KV cache of fixed capacity per sequence (``k`` / ``v`` = the cache viewed as ``[B * capacity, Hkv, D]``,
  ``cu_seqlens_k`` = multiples of the capacity) whose valid lengths live on the device: ONE captured graph serves every length, a replay follows lengths written
  in place, and with one token per sequence under GQA the group's heads are packed into the rows of one tile (FlashAttention's ``cache_seqlens`` decode).

  ``num_splits``: 0 = the library decides (launches that leave most of the chip idle — a decode batch of a few long sequences, a prefill chunk of one long
  prompt with a few heads per GPU — split every row tile's KV range over several workgroups and merge fp32 partials in a second kernel of the same call: equal
  to the unsplit launch to rounding, not to the bit), 1 = never, n = at most n.  ``FFPA_HIP_DETERMINISTIC=1`` / ``FLAG_DETERMINISTIC``: never.

  ``block_table`` (int32 device ``[B, pages_per_row]``): a PAGED KV cache — ``k`` / ``v`` are page pools ``[num_pages, page_size, Hkv, D]`` (``page_size`` a multiple
  of 64), key j of sequence i is row ``j % page_size`` of page ``block_table[i, j // page_size]``; ``seqused_k`` is required and gives the lengths (clamped to
  ``pages_per_row * page_size``), ``cu_seqlens_k`` is ignored (may be None).  One launch of the paged twin of the packed kernel (``ffpa_attn_varlen_paged_fwd``):
  no gather, nothing read back to the host, graph-capturable; replays follow ``seqused_k`` / ``block_table`` written in place.

  ``tree_words`` (int64 device ``[B | 1, tokens]``, ``max_seqlen_q <= tokens <= 64``; ``tree_forward`` is this call with it): a TREE MASK over the last keys of
  every sequence (``ffpa_attn_varlen_tree_fwd``) — token t of sequence i sees every key in front of its sequence's last ``ntok_i`` keys and, of those, key j iff
  bit j of ``tree_words[i, t]`` is set; ``causal`` is ignored.  The same kernel and plan as the causal launch; a replay follows words written in place.

  ``window`` (``(left, right)``, ints >= -1, -1 = unbounded; ``window_forward`` is this call with it): a SLIDING WINDOW (``ffpa_attn_varlen_window_fwd``) — token t
  of sequence i, at position ``pos = t + L_i - ntok_i``, sees key j iff ``pos - left <= j <= pos + right``; ``causal`` means ``right = 0``.  The KV tiles in front
  of a row tile's window are not read, and the plan prices the window's keys instead of ``max_seqlen_k``.

  ``softcap`` (a finite float > 0; ``softcap_forward`` is this call with it; 0 = none): LOGIT SOFT-CAPPING (``ffpa_attn_varlen_softcap_fwd``) — the scores are
  ``softcap * tanh(softmax_scale * q.k / softcap)``, masked behind the cap; with or without ``window`` (None = ``(-1, -1)``), whose plan the launch runs."""
  paged = block_table is not None
  tree = tree_words is not None
  capped = softcap != 0.0
  if capped and window is None:
    window = (-1, -1)
  if window is not None:
    if tree:
      raise ValueError(f"ffpa_attn::{'_softcap' if capped else '_window'}_fwd_hip: a window and a tree mask do not combine")
  family = "softcap" if capped else "window" if window is not None else "tree" if tree else "paged" if paged else "packed"  # (a key of _VARLEN_EXPORTS)
  name = f"ffpa_attn::_{'varlen' if family == 'packed' else family}_fwd_hip"
  if not q.is_cuda:
    raise NotImplementedError(f"{name} has no implementation for device '{q.device.type}' (the HIP kernel needs a GPU tensor)")
  lib = load_library()
  if q.dtype not in _DTYPE or k.dtype != q.dtype or v.dtype != q.dtype:
    raise TypeError(f"{name} only supports fp16/bf16 q/k/v of one dtype, got {q.dtype}, {k.dtype}, {v.dtype}")
  if paged:
    if q.dim() != 3 or k.dim() != 4 or v.dim() != 4:
      raise ValueError(f"{name}: q must be packed [T, Hq, D] and k / v paged [num_pages, page_size, Hkv, D]")
  elif q.dim() != 3 or k.dim() != 3 or v.dim() != 3:
    raise ValueError(f"{name}: q/k/v must be 3-D packed [T, H, D] tensors")
  if k.shape != v.shape or k.size(-1) != q.size(2):
    raise ValueError(f"{name}: k {tuple(k.shape)} and v {tuple(v.shape)} must share their shape and q's head dim ({q.size(2)})")
  if k.size(-2) == 0 or q.size(1) % k.size(-2) != 0:
    raise ValueError(f"{name}: query num_heads ({q.size(1)}) must be a multiple of key/value num_heads ({k.size(-2)})")
  if paged:
    if k.size(1) <= 0 or k.size(1) % 64 != 0:
      raise ValueError(f"{name}: page_size ({k.size(1)}) must be a positive multiple of 64")
    if cu_seqlens_q.dtype != torch.int32 or cu_seqlens_q.dim() != 1 or cu_seqlens_q.numel() < 2 or cu_seqlens_q.device != q.device:
      raise ValueError(f"{name}: cu_seqlens_q must be a 1-D int32 tensor of length batch + 1 on q's device")
    batch = cu_seqlens_q.numel() - 1
    if seqused_k is None:
      raise ValueError(f"{name}: seqused_k is required with a block_table (it gives the key lengths)")
    if seqused_k.dtype != torch.int32 or seqused_k.dim() != 1 or seqused_k.numel() != batch or seqused_k.device != q.device:
      raise ValueError(f"{name}: seqused_k must be a 1-D int32 tensor of length batch on q's device")
    if block_table.dtype != torch.int32 or block_table.dim() != 2 or block_table.size(0) != batch or block_table.size(1) == 0 or block_table.device != q.device:
      raise ValueError(f"{name}: block_table must be a 2-D int32 tensor [batch, pages_per_seq] (pages_per_seq >= 1) on q's device")
    cu_seqlens_k = None  # (not read: the lengths are seqused_k's)
  else:
    for nm, cu in (("cu_seqlens_q", cu_seqlens_q), ("cu_seqlens_k", cu_seqlens_k)):
      if cu.dtype != torch.int32 or cu.dim() != 1 or cu.numel() < 2:
        raise ValueError(f"{name}: {nm} must be a 1-D int32 tensor of length batch + 1")
      if cu.device != q.device:
        raise ValueError(f"{name}: {nm} must be on q's device, got {cu.device} and {q.device}")
    if cu_seqlens_q.numel() != cu_seqlens_k.numel():
      raise ValueError(f"{name}: cu_seqlens_q and cu_seqlens_k must have one length")
    if seqused_k is not None and (seqused_k.dtype != torch.int32 or seqused_k.dim() != 1 or seqused_k.numel() != cu_seqlens_k.numel() - 1 or seqused_k.device != q.device):
      raise ValueError(f"{name}: seqused_k must be a 1-D int32 tensor of length batch on q's device")
    cu_seqlens_k = cu_seqlens_k.contiguous()
  if k.device != q.device or v.device != q.device:
    raise ValueError(f"{name}: q/k/v must be on one device, got {q.device}, {k.device}, {v.device}")
  Tq, Hq, D = q.shape
  if window is not None:
    if not isinstance(window, (tuple, list)) or len(window) != 2 or not all(isinstance(x, int) and not isinstance(x, bool) for x in window):
      raise TypeError(f"{name}: window must be a pair of ints (left, right), got {window!r}")
    if min(window) < -1 or max(window) > 0x7FFFFFFF:
      raise ValueError(f"{name}: window (left, right) = {tuple(window)}: each must be >= -1 (-1 = unbounded)")
    window = (int(window[0]), int(window[1]))
    if capped:
      if isinstance(softcap, bool) or not isinstance(softcap, (int, float)):
        raise TypeError(f"{name}: softcap must be a real number, got {softcap!r}")
      softcap = float(softcap)
      if not (softcap > 0.0 and softcap != float("inf")):
        raise ValueError(f"{name}: softcap = {softcap} must be finite and > 0")
  elif tree:
    if not isinstance(tree_words, torch.Tensor) or tree_words.dtype != torch.int64 or tree_words.dim() != 2 or tree_words.device != q.device:
      raise ValueError(f"{name}: tree_words must be a 2-D int64 tensor [batch or 1, tokens] on q's device")
    if tree_words.size(0) not in (1, cu_seqlens_q.numel() - 1) or not max(int(max_seqlen_q), 1) <= tree_words.size(1) <= 64:
      raise ValueError(f"{name}: tree_words {tuple(tree_words.shape)} must be [batch={cu_seqlens_q.numel() - 1} or 1, tokens] with max_seqlen_q={max_seqlen_q} <= tokens <= 64")
    if tree_words.stride(1) != 1:
      tree_words = tree_words.contiguous()
  q, k, v, Dp = _pad_head_dim(q, k, v)  # (a paged call: copies the pools)
  if k.size(0) == 0:
    # no key row anywhere (an empty pool: ids clamp into this one zero page): every output row is the empty row (O = 0, LSE = -inf).  The C-ABI wants non-NULL
    # bases; nothing is read through them
    k = v = q.new_zeros((1, *k.shape[1:-1], Dp))
  q, k, v = _rows(q, 0), _rows(k, -3), _rows(v, -3)  # (k / v: [T, H, D] rows or [num_pages, page_size, H, D] pools — the row axis is the third from the end)
  cu_seqlens_q = cu_seqlens_q.contiguous()
  if seqused_k is not None:
    seqused_k = seqused_k.contiguous()
  o = torch.empty((Tq, Hq, Dp), dtype=q.dtype, device=q.device)
  lse = torch.empty((Hq, Tq), dtype=torch.float32, device=q.device) if return_lse else None
  if Tq == 0 or max_seqlen_q <= 0:
    return (o[..., :D] if Dp != D else o), lse  # (nothing to compute: no query row in any sequence)
  # (a pool's k_stride / v_stride are {row, head} inside a page)
  p = _varlen_params(q.dtype, cu_seqlens_q.numel() - 1, Hq, k.size(-2), Dp, max_seqlen_q, max_seqlen_k, Tq, [t.stride()[-3:-1] for t in (q, k, v, o)], causal, softmax_scale,
                     rescale_threshold, int(flags) | _deterministic_flag(), num_splits)
  p.q, p.k, p.v, p.o = q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr()
  p.lse = lse.data_ptr() if lse is not None else None
  p.lse_stride_head = lse.stride(0) if lse is not None else 0
  p.cu_seqlens_q = cu_seqlens_q.data_ptr()
  p.cu_seqlens_kv = cu_seqlens_k.data_ptr() if cu_seqlens_k is not None else None
  p.seqused_kv = seqused_k.data_ptr() if seqused_k is not None else None
  kv = None
  args = (ctypes.byref(p),)
  if paged:
    kv, block_table = _paged_kv_of(block_table, k, v)
    args = (ctypes.byref(p), ctypes.byref(kv))
  if window is not None:
    wn = _stamped(FfpaWindow)
    wn.left, wn.right = window
    args = (ctypes.byref(p), ctypes.byref(kv) if paged else None, ctypes.byref(wn))
    if capped:
      args += (ctypes.c_float(softcap),)
  elif tree:
    tm = _stamped(FfpaTreeMask)
    tm.bits, tm.tokens = tree_words.data_ptr(), tree_words.size(1)
    tm.batch_stride = tree_words.stride(0) if tree_words.size(0) > 1 else 0
    args = (ctypes.byref(p), ctypes.byref(kv) if paged else None, ctypes.byref(tm))
  with torch.cuda.device(q.device):
    stream = torch.cuda.current_stream(q.device).cuda_stream
    workspace = _hand_over_workspace(p, q.device, stream, _varlen_scratch(lib, p, q.device.index or 0, family, paged, args, window))  # (the cap changes no plan: the key needs no softcap)  # (held in a local until the launch below has been enqueued)
    if plan_out is not None:
      plan_out.update(_read_plan(lib, _varlen_fn(lib, family, "_plan"), _varlen_fn(lib, family, "_kernel"), _VARLEN_PLAN_KEYS, args))
    rc = _varlen_fn(lib, family)(*args, ctypes.c_void_p(stream))
  if rc != 0:
    _raise_status(lib, rc, _VARLEN_EXPORTS[family])
  return _unpad_head_dim(o, D), lse


def tree_forward(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, cu_seqlens_q: torch.Tensor, cu_seqlens_k: "torch.Tensor | None", max_seqlen_q: int,
                 max_seqlen_k: int, softmax_scale: float, tree_words: torch.Tensor, *, rescale_threshold: float = -1.0, return_lse: bool = True, flags: int = 0,
                 plan_out: "dict | None" = None, seqused_k: "torch.Tensor | None" = None, num_splits: int = 0, block_table: "torch.Tensor | None" = None):
  """One launch of the packed-sequence kernel (``block_table``: of its paged twin) under a TREE MASK (``ffpa_attn_varlen_tree_fwd``; ``varlen_forward``'s
  ``tree_words``): ``tree_words`` int64 ``[B | 1, tokens]`` as ``ffpa_attn_amd.pack_tree_mask`` makes them.  ``flags`` / ``plan_out`` as ``varlen_forward``
  (``FLAG_NO_PACK_GQA``, ``FLAG_KV_STREAM``, the split count: tests force or inspect the launch)."""
  if tree_words is None:
    raise ValueError("ffpa_attn::_tree_fwd_hip: tree_words is required")
  return varlen_forward(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, True, softmax_scale, rescale_threshold=rescale_threshold,
                        return_lse=return_lse, flags=flags, plan_out=plan_out, seqused_k=seqused_k, num_splits=num_splits, block_table=block_table,
                        tree_words=tree_words)


def window_forward(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, cu_seqlens_q: torch.Tensor, cu_seqlens_k: "torch.Tensor | None", max_seqlen_q: int,
                   max_seqlen_k: int, causal: bool, softmax_scale: float, window: "tuple[int, int]", *, rescale_threshold: float = -1.0, return_lse: bool = True,
                   flags: int = 0, plan_out: "dict | None" = None, seqused_k: "torch.Tensor | None" = None, num_splits: int = 0,
                   block_table: "torch.Tensor | None" = None):
  """One launch of the packed-sequence kernel (``block_table``: of its paged twin) under a SLIDING WINDOW (``ffpa_attn_varlen_window_fwd``; ``varlen_forward``'s
  ``window``).  ``flags`` / ``plan_out`` as ``varlen_forward`` (tests force or inspect the launch)."""
  if window is None:
    raise ValueError("ffpa_attn::_window_fwd_hip: window is required")
  return varlen_forward(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, causal, softmax_scale, rescale_threshold=rescale_threshold,
                        return_lse=return_lse, flags=flags, plan_out=plan_out, seqused_k=seqused_k, num_splits=num_splits, block_table=block_table,
                        window=window)


def softcap_forward(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, cu_seqlens_q: torch.Tensor, cu_seqlens_k: "torch.Tensor | None", max_seqlen_q: int,
                    max_seqlen_k: int, causal: bool, softmax_scale: float, softcap: float, window: "tuple[int, int]" = (-1, -1), *, rescale_threshold: float = -1.0,
                    return_lse: bool = True, flags: int = 0, plan_out: "dict | None" = None, seqused_k: "torch.Tensor | None" = None, num_splits: int = 0,
                    block_table: "torch.Tensor | None" = None):
  """One launch of the packed-sequence kernel (``block_table``: of its paged twin) with LOGIT SOFT-CAPPING, under ``window`` (``ffpa_attn_varlen_softcap_fwd``;
  ``varlen_forward``'s ``softcap``).  ``flags`` / ``plan_out`` as ``varlen_forward`` (tests force or inspect the launch)."""
  if isinstance(softcap, bool) or not isinstance(softcap, (int, float)):
    raise TypeError(f"ffpa_attn::_softcap_fwd_hip: softcap must be a real number, got {softcap!r}")
  if not (softcap > 0.0 and softcap != float("inf")):
    raise ValueError(f"ffpa_attn::_softcap_fwd_hip: softcap = {softcap} must be finite and > 0")
  return varlen_forward(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, causal, softmax_scale, rescale_threshold=rescale_threshold,
                        return_lse=return_lse, flags=flags, plan_out=plan_out, seqused_k=seqused_k, num_splits=num_splits, block_table=block_table,
                        window=window, softcap=float(softcap))


def varlen_launch_plan(batch: int, heads_q: int, heads_kv: int, max_seqlen_q: int, max_seqlen_k: int, head_dim: int, *,
                       dtype: torch.dtype = torch.bfloat16, causal: bool = False, flags: int = 0, total_q: int = 0, num_splits: int = 0,
                       page_size: int = 0, window: "tuple[int, int] | None" = None, softcap: float = 0.0) -> dict:
  """The packed-sequence launch for a shape class, without launching (placeholder pointers): row tiles per (sequence, head), tile, workgroups, KV ranges per
  sequence, kernel name.  ``total_q`` (rows of q) > 0: the plan of a call that hands the library its scratch (``varlen_forward`` does) — KV splits included;
  0: the plan without scratch (never split).  ``page_size`` > 0: the paged call's plan (``ffpa_attn_varlen_paged_fwd``, a table of one page per sequence row
  covering max_seqlen_k).  ``window`` = (left, right): the sliding-window call's plan (``ffpa_attn_varlen_window_fwd``), priced at the window's keys.
  ``softcap`` > 0: the soft-capping call's (``ffpa_attn_varlen_softcap_fwd``: the window call's plan, ``window`` None = no window, and the capped kernel's name)."""
  lib = load_library()
  d8 = (int(head_dim) + 7) // 8 * 8
  strides = [(h * d8, d8) for h in (heads_q, heads_kv, heads_kv, heads_q)]
  p = _varlen_params(dtype, int(batch), int(heads_q), int(heads_kv), d8, max_seqlen_q, max_seqlen_k, int(total_q), strides, causal, float(head_dim) ** -0.5, -1.0, flags, num_splits)
  p.q = p.k = p.v = p.o = p.cu_seqlens_q = p.cu_seqlens_kv = 16
  if total_q > 0:
    p.workspace, p.workspace_bytes = 16, 0xFFFFFFFFFFFFFFFF
  kv, fam = None, "packed"
  args = (ctypes.byref(p),)
  if page_size:
    fam = "paged"
    p.seqused_kv = 16
    pages_per_row = max(1, -(-int(max_seqlen_k) // int(page_size)))
    kv = _paged_kv(16, pages_per_row, pages_per_row, int(page_size), int(batch) * pages_per_row, int(page_size) * heads_kv * d8, int(page_size) * heads_kv * d8)
    args = (ctypes.byref(p), ctypes.byref(kv))
  if softcap and window is None:
    window = (-1, -1)
  if window is not None:
    wn = _stamped(FfpaWindow)
    wn.left, wn.right = int(window[0]), int(window[1])
    args, fam = (ctypes.byref(p), ctypes.byref(kv) if kv is not None else None, ctypes.byref(wn)), "window"
    if softcap:
      args, fam = args + (ctypes.c_float(softcap),), "softcap"
  out = _read_plan(lib, _varlen_fn(lib, fam, "_plan"), _varlen_fn(lib, fam, "_kernel"), _VARLEN_PLAN_KEYS, args, strict=True)
  if total_q <= 0:
    del out["splits"]
  return out


torch.library.define(
  f"{_OP_NAMESPACE}::_varlen_fwd_hip",
  "(Tensor q, Tensor k, Tensor v, Tensor cu_seqlens_q, Tensor cu_seqlens_k, int max_seqlen_q, int max_seqlen_k, "
  "float softmax_scale, int causal, float rescale_threshold=-1.0, Tensor? seqused_k=None) -> (Tensor o, Tensor softmax_lse)",
)


@torch.library.impl(f"{_OP_NAMESPACE}::_varlen_fwd_hip", "CUDA")  # ROCm tensors dispatch on the CUDA key
def _varlen_fwd_hip_torch_op(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, softmax_scale, causal, rescale_threshold=-1.0, seqused_k=None):
  return varlen_forward(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, bool(causal), softmax_scale,
                        rescale_threshold=rescale_threshold, return_lse=True, seqused_k=seqused_k)


@torch.library.register_fake(f"{_OP_NAMESPACE}::_varlen_fwd_hip")
def _packed_out_fake(q, *args, **kwargs):
  """The fake of the five attention ops over packed q (packed, paged, tree, window, softcap): ``q [T, Hq, D]`` -> ``(o [T, Hq, D], lse [Hq, T] fp32)``."""
  total_q, heads, head_dim = q.shape
  return q.new_empty((total_q, heads, head_dim)), q.new_empty((heads, total_q), dtype=torch.float32)


# The paged-KV call (ffpa_attn_with_kvcache(block_table=...)): its own op, so that the packed op's schema stays the reference's
torch.library.define(
  f"{_OP_NAMESPACE}::_paged_fwd_hip",
  "(Tensor q, Tensor k, Tensor v, Tensor cu_seqlens_q, Tensor seqused_k, Tensor block_table, int max_seqlen_q, int max_seqlen_k, "
  "float softmax_scale, int causal, float rescale_threshold=-1.0, int num_splits=0) -> (Tensor o, Tensor softmax_lse)",
)


@torch.library.impl(f"{_OP_NAMESPACE}::_paged_fwd_hip", "CUDA")  # ROCm tensors dispatch on the CUDA key
def _paged_fwd_hip_torch_op(q, k, v, cu_seqlens_q, seqused_k, block_table, max_seqlen_q, max_seqlen_k, softmax_scale, causal, rescale_threshold=-1.0, num_splits=0):
  return varlen_forward(q, k, v, cu_seqlens_q, None, max_seqlen_q, max_seqlen_k, bool(causal), softmax_scale,
                        rescale_threshold=rescale_threshold, return_lse=True, seqused_k=seqused_k, num_splits=num_splits, block_table=block_table)


torch.library.register_fake(f"{_OP_NAMESPACE}::_paged_fwd_hip", _packed_out_fake)


# The tree-mask call (ffpa_attn_with_kvcache_tree): one op for both caches — ``block_table`` None = the contiguous cache as packed rows + ``cu_seqlens_k``
torch.library.define(
  f"{_OP_NAMESPACE}::_tree_fwd_hip",
  "(Tensor q, Tensor k, Tensor v, Tensor cu_seqlens_q, Tensor? cu_seqlens_k, Tensor seqused_k, Tensor? block_table, Tensor tree_words, int max_seqlen_q, "
  "int max_seqlen_k, float softmax_scale, float rescale_threshold=-1.0, int num_splits=0) -> (Tensor o, Tensor softmax_lse)",
)


@torch.library.impl(f"{_OP_NAMESPACE}::_tree_fwd_hip", "CUDA")  # ROCm tensors dispatch on the CUDA key
def _tree_fwd_hip_torch_op(q, k, v, cu_seqlens_q, cu_seqlens_k, seqused_k, block_table, tree_words, max_seqlen_q, max_seqlen_k, softmax_scale,
                           rescale_threshold=-1.0, num_splits=0):
  return tree_forward(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, softmax_scale, tree_words, rescale_threshold=rescale_threshold,
                      return_lse=True, seqused_k=seqused_k, num_splits=num_splits, block_table=block_table)


torch.library.register_fake(f"{_OP_NAMESPACE}::_tree_fwd_hip", _packed_out_fake)


# The sliding-window call (ffpa_attn_with_kvcache_window): one op for both caches, shaped like the tree call's — ``block_table`` None = the contiguous cache
torch.library.define(
  f"{_OP_NAMESPACE}::_window_fwd_hip",
  "(Tensor q, Tensor k, Tensor v, Tensor cu_seqlens_q, Tensor? cu_seqlens_k, Tensor seqused_k, Tensor? block_table, int window_left, int window_right, "
  "int max_seqlen_q, int max_seqlen_k, float softmax_scale, int causal, float rescale_threshold=-1.0, int num_splits=0) -> (Tensor o, Tensor softmax_lse)",
)


@torch.library.impl(f"{_OP_NAMESPACE}::_window_fwd_hip", "CUDA")  # ROCm tensors dispatch on the CUDA key
def _window_fwd_hip_torch_op(q, k, v, cu_seqlens_q, cu_seqlens_k, seqused_k, block_table, window_left, window_right, max_seqlen_q, max_seqlen_k, softmax_scale,
                             causal, rescale_threshold=-1.0, num_splits=0):
  return window_forward(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, bool(causal), softmax_scale, (int(window_left), int(window_right)),
                        rescale_threshold=rescale_threshold, return_lse=True, seqused_k=seqused_k, num_splits=num_splits, block_table=block_table)


torch.library.register_fake(f"{_OP_NAMESPACE}::_window_fwd_hip", _packed_out_fake)


# The soft-capping call (ffpa_attn_with_kvcache_softcap): the window call's op with the cap — ``block_table`` None = the contiguous cache, (-1, -1) = no window
torch.library.define(
  f"{_OP_NAMESPACE}::_softcap_fwd_hip",
  "(Tensor q, Tensor k, Tensor v, Tensor cu_seqlens_q, Tensor? cu_seqlens_k, Tensor seqused_k, Tensor? block_table, float softcap, int window_left, "
  "int window_right, int max_seqlen_q, int max_seqlen_k, float softmax_scale, int causal, float rescale_threshold=-1.0, int num_splits=0) -> "
  "(Tensor o, Tensor softmax_lse)",
)


@torch.library.impl(f"{_OP_NAMESPACE}::_softcap_fwd_hip", "CUDA")  # ROCm tensors dispatch on the CUDA key
def _softcap_fwd_hip_torch_op(q, k, v, cu_seqlens_q, cu_seqlens_k, seqused_k, block_table, softcap, window_left, window_right, max_seqlen_q, max_seqlen_k,
                              softmax_scale, causal, rescale_threshold=-1.0, num_splits=0):
  return softcap_forward(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, bool(causal), softmax_scale, float(softcap),
                         (int(window_left), int(window_right)), rescale_threshold=rescale_threshold, return_lse=True, seqused_k=seqused_k, num_splits=num_splits,
                         block_table=block_table)


torch.library.register_fake(f"{_OP_NAMESPACE}::_softcap_fwd_hip", _packed_out_fake)


# The MLA latent-cache call (ffpa_attn_with_kvcache_mla): ONE pool whose rows are the keys and, in their first ``head_dim_v`` columns, the values
MLA_BUILDS = ((576, 512),)  # the (head dim, value width) pairs the library carries (csrc/ffpa_mla.h FFPA_FOR_EACH_MLA_BUILD)
_MLA_SCRATCH: "dict[tuple, int]" = {}


def mla_row_chunks(group: int, seqlen_q: int, block_rows: int = 64) -> "list[list[tuple[int, int]]]":
  """The launch's row packing as a pure function: the ``group`` query heads of a KV head x the ``seqlen_q`` tokens of a sequence are the rows of its tiles,
  head-major (row r = (head r // seqlen_q, token r % seqlen_q)), cut into ``ceil(group * seqlen_q / block_rows)`` chunks of at most ``block_rows`` rows — the row
  tiles of one (sequence, KV head), neighbours in the launch order.  -> the (head in group, token) rows of every chunk.  ``group`` = 1 does not pack: rows are
  tokens, and the chunks are its row tiles all the same."""
  rows = [(r // seqlen_q, r % seqlen_q) for r in range(group * seqlen_q)]
  return [rows[i:i + block_rows] for i in range(0, len(rows), block_rows)]


def mla_ragged_row_chunks(group: int, seqlens_q: "list[int]", block_rows: int = 64) -> "tuple[list[list[list[tuple[int, int]]]], int]":
  """``mla_row_chunks`` for a RAGGED batch: sequence b brings ``seqlens_q[b]`` tokens, and its ``group * seqlens_q[b]`` packed rows are cut into its own
  ``ceil(group * seqlens_q[b] / block_rows)`` chunks (none for an empty sequence) -> ``(the chunks of every sequence, slots)``.  ``slots`` =
  ``ceil(group * sum(seqlens_q) / block_rows) + len(seqlens_q)``: the row-tile slots per KV head of the compact grid, an upper bound of the number of chunks
  (every sequence rounds up by less than one tile).  The plan takes the compact grid when ``4 * slots <= len(seqlens_q) * ceil(group * max(seqlens_q) /
  block_rows)`` — the full grid's row tiles per KV head — and the rows are packed over more than one tile (``group > 1``, ``group * max(seqlens_q) > block_rows``)."""
  chunks = [mla_row_chunks(group, n, block_rows) if n > 0 else [] for n in seqlens_q]
  return chunks, -(-group * sum(seqlens_q) // block_rows) + len(seqlens_q)


def mla_compact_slots(group: int, seqlens_q: "list[int]", block_rows: int = 64) -> int:
  """The plan's compact-grid decision for packed latent rows as a pure function (``mla_ragged_row_chunks``' rule) -> the slots per KV head, or 0 for the full grid."""
  slots = mla_ragged_row_chunks(group, seqlens_q, block_rows)[1]
  nqt = -(-group * max(seqlens_q) // block_rows)
  return slots if group > 1 and nqt > 1 and sum(seqlens_q) > 0 and 4 * slots <= len(seqlens_q) * nqt else 0


def mla_forward(q: torch.Tensor, kv_cache: torch.Tensor, head_dim_v: int, cu_seqlens_q: torch.Tensor, seqused_k: torch.Tensor, block_table: torch.Tensor,
                max_seqlen_q: int, max_seqlen_k: int, causal: bool, softmax_scale: float, *, kv_new: "torch.Tensor | None" = None,
                cache_seqlens: "torch.Tensor | None" = None, return_lse: bool = True, flags: int = 0, plan_out: "dict | None" = None, num_splits: int = 0,
                tree_words: "torch.Tensor | None" = None, kv_scale: "float | None" = None):
  """One call of ``ffpa_attn_varlen_mla_fwd``: ``q [T, Hq, D]`` packed by ``cu_seqlens_q``, the latent pool ``kv_cache [num_pages, page_size, Hkv, D]`` (written in
  place by the append) with its int32 ``block_table [B, pages_per_seq]`` -> ``(o [T, Hq, head_dim_v], lse [Hq, T] fp32 | None)``.  The keys of KV head h are
  ``kv_cache[..., h, :]``, its values ``kv_cache[..., h, :head_dim_v]``.  ``seqused_k`` int32 ``[B]``: the key lengths — or, with ``kv_new [B, Snew, Hkv, D]``, the
  buffer that RECEIVES ``min(max(cache_seqlens, 0) + Snew, capacity)`` from the append launch in front of the attention launch (``cache_seqlens``: the lengths
  before the step).  Nothing is read back to the host: the call captures into a HIP graph.  ``flags`` / ``plan_out`` / ``num_splits`` as ``varlen_forward``.

  ``tree_words`` (int64 device ``[B | 1, tokens]``, ``max_seqlen_q <= tokens <= 64``; ``mla_tree_forward`` is this call with it): a TREE MASK over the last rows
  of every sequence (``ffpa_attn_varlen_mla_tree_fwd``, its own kernel) — token t of sequence i sees every row in front of its sequence's last ``ntok_i`` rows and,
  of those, row j iff bit j of ``tree_words[i, t]`` is set; ``causal`` is ignored: the launch and its plan are the causal latent launch's.

  ``kv_scale`` (a host float, finite and > 0; ``mla_fp8_forward`` is this call with it): the pool is ``torch.float8_e4m3fn`` — OCP e4m3 codes, K = kv_scale x K8 —
  and the call is ``ffpa_attn_varlen_mla_fp8_fwd``, its own kernel; q, ``kv_new`` (quantised by the append, ``quantize_latent_rows``' definition) and o stay
  bf16 / fp16.  With ``tree_words`` as well (``mla_tree_fp8_forward``): ``ffpa_attn_varlen_mla_tree_fp8_fwd``, the tree mask over the FP8 pool."""
  tree = tree_words is not None
  fp8 = kv_scale is not None
  kind = ("_tree" if tree else "") + ("_fp8" if fp8 else "")
  name = f"ffpa_attn::_mla{kind}_fwd_hip"
  export = f"ffpa_attn_varlen_mla{kind}_fwd"
  if not q.is_cuda:
    raise NotImplementedError(f"{name} has no implementation for device '{q.device.type}' (the HIP kernel needs a GPU tensor)")
  lib = load_library()
  if fp8:
    if q.dtype not in _DTYPE or kv_cache.dtype != torch.float8_e4m3fn:
      raise TypeError(f"{name} only supports fp16/bf16 q over a torch.float8_e4m3fn kv_cache (OCP e4m3, the chip's FP8 format), got {q.dtype}, {kv_cache.dtype}")
    kv_scale = check_kv_scale(kv_scale, name)
  elif q.dtype not in _DTYPE or kv_cache.dtype != q.dtype:
    raise TypeError(f"{name} only supports fp16/bf16 q/kv_cache of one dtype, got {q.dtype}, {kv_cache.dtype}")
  if q.dim() != 3 or kv_cache.dim() != 4 or kv_cache.size(-1) != q.size(2):
    raise ValueError(f"{name}: q must be packed [T, Hq, D] and kv_cache paged [num_pages, page_size, Hkv, D] of q's head dim")
  Tq, Hq, D = q.shape
  if (D, int(head_dim_v)) not in MLA_BUILDS:
    raise NotImplementedError(f"{name}: (head_dim, head_dim_v) = ({D}, {head_dim_v}) is not built (built: {', '.join(map(str, MLA_BUILDS))})")
  if kv_cache.size(2) == 0 or Hq % kv_cache.size(2) != 0:
    raise ValueError(f"{name}: query num_heads ({Hq}) must be a multiple of the latent num_heads ({kv_cache.size(2)})")
  if kv_cache.size(1) <= 0 or kv_cache.size(1) % 64 != 0:
    raise ValueError(f"{name}: page_size ({kv_cache.size(1)}) must be a positive multiple of 64")
  if cu_seqlens_q.dtype != torch.int32 or cu_seqlens_q.dim() != 1 or cu_seqlens_q.numel() < 2 or cu_seqlens_q.device != q.device:
    raise ValueError(f"{name}: cu_seqlens_q must be a 1-D int32 tensor of length batch + 1 on q's device")
  batch = cu_seqlens_q.numel() - 1
  for nm, t in (("seqused_k", seqused_k),) + ((("cache_seqlens", cache_seqlens),) if kv_new is not None else ()):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.dim() != 1 or t.numel() != batch or t.device != q.device:
      raise ValueError(f"{name}: {nm} must be a 1-D int32 tensor of length batch on q's device")
  if block_table.dtype != torch.int32 or block_table.dim() != 2 or block_table.size(0) != batch or block_table.size(1) == 0 or block_table.device != q.device:
    raise ValueError(f"{name}: block_table must be a 2-D int32 tensor [batch, pages_per_seq] (pages_per_seq >= 1) on q's device")
  if kv_cache.device != q.device or kv_cache.size(0) == 0:
    raise ValueError(f"{name}: kv_cache must be a non-empty pool on q's device")
  if not _layout_ok(kv_cache, -3) or (fp8 and any(st % 16 for st in kv_cache.stride()[:-1])):
    raise ValueError(f"{name}: kv_cache needs head-dim stride 1, strides that are multiples of {16 if fp8 else 8} elements and a 16-byte aligned base (it is read, and "
                     "written, in place)")
  if tree:
    if not isinstance(tree_words, torch.Tensor) or tree_words.dtype != torch.int64 or tree_words.dim() != 2 or tree_words.device != q.device:
      raise ValueError(f"{name}: tree_words must be a 2-D int64 tensor [batch or 1, tokens] on q's device")
    if tree_words.size(0) not in (1, batch) or not max(int(max_seqlen_q), 1) <= tree_words.size(1) <= 64:
      raise ValueError(f"{name}: tree_words {tuple(tree_words.shape)} must be [batch={batch} or 1, tokens] with max_seqlen_q={max_seqlen_q} <= tokens <= 64")
    if tree_words.stride(1) != 1:
      tree_words = tree_words.contiguous()
    causal = True
  q = _rows(q, 0)
  cu_seqlens_q, seqused_k = cu_seqlens_q.contiguous(), seqused_k if seqused_k.is_contiguous() else seqused_k.contiguous()
  o = torch.empty((Tq, Hq, int(head_dim_v)), dtype=q.dtype, device=q.device)
  lse = torch.empty((Hq, Tq), dtype=torch.float32, device=q.device) if return_lse else None
  if Tq == 0 or max_seqlen_q <= 0:
    return o, lse
  ks = kv_cache.stride()[-3:-1]
  p = _varlen_params(q.dtype, batch, Hq, kv_cache.size(2), D, max_seqlen_q, max_seqlen_k, Tq, [q.stride()[-3:-1], ks, ks, o.stride()[-3:-1]], causal, softmax_scale,
                     -1.0, int(flags) | _deterministic_flag(), num_splits)
  p.q, p.k, p.v, p.o = q.data_ptr(), kv_cache.data_ptr(), kv_cache.data_ptr(), o.data_ptr()
  p.lse = lse.data_ptr() if lse is not None else None
  p.lse_stride_head = lse.stride(0) if lse is not None else 0
  p.cu_seqlens_q = cu_seqlens_q.data_ptr()
  p.seqused_kv = seqused_k.data_ptr()
  kv, block_table = _paged_kv_of(block_table, kv_cache, kv_cache)
  m = _stamped(FfpaMla)
  m.head_dim_v = int(head_dim_v)
  if kv_new is not None:
    if kv_new.dtype != q.dtype or kv_new.device != q.device or kv_new.dim() != 4 or kv_new.size(0) != batch or tuple(kv_new.shape[2:]) != tuple(kv_cache.shape[2:]):
      raise ValueError(f"{name}: kv_new must be [B={batch}, Snew, Hkv={kv_cache.size(2)}, D={D}] of q's dtype on q's device, got {tuple(kv_new.shape)}")
    kv_new = _rows(kv_new)
    cache_seqlens = cache_seqlens.contiguous()
    if cache_seqlens.data_ptr() == seqused_k.data_ptr():
      raise ValueError(f"{name}: seqused_k receives the post-append lengths and must not be cache_seqlens")
    m.seqlen_new, m.kv_new, m.cache_seqlens = kv_new.size(1), kv_new.data_ptr(), cache_seqlens.data_ptr()
    m.kv_new_stride[:] = list(kv_new.stride()[:3])
  args = (ctypes.byref(p), ctypes.byref(kv), ctypes.byref(m))
  if tree:
    tm = _stamped(FfpaTreeMask)
    tm.bits, tm.tokens = tree_words.data_ptr(), tree_words.size(1)
    tm.batch_stride = tree_words.stride(0) if tree_words.size(0) > 1 else 0
    args += (ctypes.byref(tm),)
  if fp8:  # (behind the mask: the order of the C calls' arguments)
    f8 = _stamped(FfpaMlaFp8)
    f8.kv_scale = kv_scale
    args += (ctypes.byref(f8),)
  with torch.cuda.device(q.device):
    stream = torch.cuda.current_stream(q.device).cuda_stream
    nbytes = 0
    if not (p.num_splits == 1 or p.flags & FLAG_DETERMINISTIC):
      key = (id(lib), q.device.index or 0, p.dtype, batch, Hq, p.heads_kv, D, m.head_dim_v, p.max_seqlen_q, p.max_seqlen_kv, Tq, p.causal, p.flags, p.num_splits,
             os.environ.get("FFPA_HIP_FAKE_CUS"), tm.tokens if tree else 0, fp8)
      nbytes = _cached_scratch(_MLA_SCRATCH, key, lambda: int(getattr(lib, export + "_workspace_bytes")(*args)))
    workspace = _hand_over_workspace(p, q.device, stream, nbytes)  # (held in a local until the launch below has been enqueued)
    if plan_out is not None:
      plan_out.update(_read_plan(lib, getattr(lib, export + "_plan"), getattr(lib, export + "_kernel"), _VARLEN_PLAN_KEYS, args))
      slots = ctypes.c_int(0)
      if hasattr(lib, export + "_compact_slots") and getattr(lib, export + "_compact_slots")(*args, ctypes.byref(slots)) == 0:
        plan_out["compact_slots"] = slots.value  # (row-tile slots per KV head of the compact grid; 0: the full grid)
    rc = getattr(lib, export)(*args, ctypes.c_void_p(stream))
  if rc != 0:
    _raise_status(lib, rc, export)
  return o, lse


def mla_tree_forward(q: torch.Tensor, kv_cache: torch.Tensor, head_dim_v: int, cu_seqlens_q: torch.Tensor, seqused_k: torch.Tensor, block_table: torch.Tensor,
                     max_seqlen_q: int, max_seqlen_k: int, softmax_scale: float, tree_words: torch.Tensor, *, kv_new: "torch.Tensor | None" = None,
                     cache_seqlens: "torch.Tensor | None" = None, return_lse: bool = True, flags: int = 0, plan_out: "dict | None" = None, num_splits: int = 0):
  """One call of ``ffpa_attn_varlen_mla_tree_fwd`` — the latent call under a TREE MASK (``mla_forward``'s ``tree_words``): ``tree_words`` int64 ``[B | 1, tokens]`` as
  ``ffpa_attn_amd.pack_tree_mask`` makes them.  ``kv_new`` / ``cache_seqlens`` / ``flags`` / ``plan_out`` / ``num_splits`` as ``mla_forward`` (tests force or inspect
  the launch)."""
  if tree_words is None:
    raise ValueError("ffpa_attn::_mla_tree_fwd_hip: tree_words is required")
  return mla_forward(q, kv_cache, head_dim_v, cu_seqlens_q, seqused_k, block_table, max_seqlen_q, max_seqlen_k, True, softmax_scale, kv_new=kv_new,
                     cache_seqlens=cache_seqlens, return_lse=return_lse, flags=flags, plan_out=plan_out, num_splits=num_splits, tree_words=tree_words)


def check_kv_scale(kv_scale, name: str) -> float:
  """``kv_scale`` of the FP8 latent calls -> a float: a host real number, finite and positive (a tensor would need a read-back: ``TypeError``)."""
  if isinstance(kv_scale, torch.Tensor):
    raise TypeError(f"{name}: kv_scale must be a host float, not a tensor (a device scalar would need a read-back to the host)")
  if isinstance(kv_scale, bool) or not isinstance(kv_scale, (int, float)):
    raise TypeError(f"{name}: kv_scale must be a real number, got {kv_scale!r}")
  kv_scale = float(kv_scale)
  if not math.isfinite(kv_scale) or not kv_scale > 0.0 or not math.isfinite(1.0 / kv_scale):
    raise ValueError(f"{name}: kv_scale must be finite and > 0 (K = kv_scale * K8), got {kv_scale!r}")
  return kv_scale


def mla_fp8_forward(q: torch.Tensor, kv_cache: torch.Tensor, head_dim_v: int, cu_seqlens_q: torch.Tensor, seqused_k: torch.Tensor, block_table: torch.Tensor,
                    max_seqlen_q: int, max_seqlen_k: int, causal: bool, softmax_scale: float, kv_scale: float, *, kv_new: "torch.Tensor | None" = None,
                    cache_seqlens: "torch.Tensor | None" = None, return_lse: bool = True, flags: int = 0, plan_out: "dict | None" = None, num_splits: int = 0):
  """One call of ``ffpa_attn_varlen_mla_fp8_fwd`` — the latent call over a ``torch.float8_e4m3fn`` pool with the per-tensor ``kv_scale`` (``mla_forward``'s
  ``kv_scale``).  ``kv_new`` / ``cache_seqlens`` / ``flags`` / ``plan_out`` / ``num_splits`` as ``mla_forward`` (tests force or inspect the launch)."""
  if kv_scale is None:
    raise ValueError("ffpa_attn::_mla_fp8_fwd_hip: kv_scale is required")
  return mla_forward(q, kv_cache, head_dim_v, cu_seqlens_q, seqused_k, block_table, max_seqlen_q, max_seqlen_k, causal, softmax_scale, kv_new=kv_new,
                     cache_seqlens=cache_seqlens, return_lse=return_lse, flags=flags, plan_out=plan_out, num_splits=num_splits, kv_scale=kv_scale)


def mla_tree_fp8_forward(q: torch.Tensor, kv_cache: torch.Tensor, head_dim_v: int, cu_seqlens_q: torch.Tensor, seqused_k: torch.Tensor, block_table: torch.Tensor,
                         max_seqlen_q: int, max_seqlen_k: int, softmax_scale: float, tree_words: torch.Tensor, kv_scale: float, *,
                         kv_new: "torch.Tensor | None" = None, cache_seqlens: "torch.Tensor | None" = None, return_lse: bool = True, flags: int = 0,
                         plan_out: "dict | None" = None, num_splits: int = 0):
  """One call of ``ffpa_attn_varlen_mla_tree_fp8_fwd`` — the latent call under a TREE MASK over a ``torch.float8_e4m3fn`` pool (``mla_forward``'s ``tree_words`` and
  ``kv_scale`` together).  ``kv_new`` (quantised by the append) / ``cache_seqlens`` / ``flags`` / ``plan_out`` / ``num_splits`` as ``mla_forward``."""
  if tree_words is None or kv_scale is None:
    raise ValueError("ffpa_attn::_mla_tree_fp8_fwd_hip: tree_words and kv_scale are required")
  return mla_forward(q, kv_cache, head_dim_v, cu_seqlens_q, seqused_k, block_table, max_seqlen_q, max_seqlen_k, True, softmax_scale, kv_new=kv_new,
                     cache_seqlens=cache_seqlens, return_lse=return_lse, flags=flags, plan_out=plan_out, num_splits=num_splits, tree_words=tree_words,
                     kv_scale=kv_scale)


# kv_cache is written in place by the append (kv_new): the schema says so
torch.library.define(
  f"{_OP_NAMESPACE}::_mla_fwd_hip",
  "(Tensor q, Tensor(a!) kv_cache, int head_dim_v, Tensor cu_seqlens_q, Tensor(b!) seqused_k, Tensor block_table, Tensor? kv_new, Tensor? cache_seqlens, "
  "int max_seqlen_q, int max_seqlen_k, float softmax_scale, int causal, int num_splits=0) -> (Tensor o, Tensor softmax_lse)",
)


@torch.library.impl(f"{_OP_NAMESPACE}::_mla_fwd_hip", "CUDA")  # ROCm tensors dispatch on the CUDA key
def _mla_fwd_hip_torch_op(q, kv_cache, head_dim_v, cu_seqlens_q, seqused_k, block_table, kv_new, cache_seqlens, max_seqlen_q, max_seqlen_k, softmax_scale, causal,
                          num_splits=0):
  return mla_forward(q, kv_cache, int(head_dim_v), cu_seqlens_q, seqused_k, block_table, max_seqlen_q, max_seqlen_k, bool(causal), softmax_scale, kv_new=kv_new,
                     cache_seqlens=cache_seqlens, return_lse=True, num_splits=num_splits)


@torch.library.register_fake(f"{_OP_NAMESPACE}::_mla_fwd_hip")
def _mla_out_fake(q, kv_cache, head_dim_v, *args, **kwargs):
  """What the four latent attention ops return (this one, its FP8, tree and sparse twins: their argument lists differ behind ``head_dim_v``)."""
  total_q, heads, _ = q.shape
  return q.new_empty((total_q, heads, head_dim_v)), q.new_empty((heads, total_q), dtype=torch.float32)


# The FP8 latent call (ffpa_attn_with_kvcache_mla_fp8 / ffpa_attn_varlen_with_kvcache_mla_fp8): the latent call's op with the per-tensor scale — kv_cache (float8_e4m3fn)
# is written in place by the quantising append (kv_new), as there
torch.library.define(
  f"{_OP_NAMESPACE}::_mla_fp8_fwd_hip",
  "(Tensor q, Tensor(a!) kv_cache, int head_dim_v, float kv_scale, Tensor cu_seqlens_q, Tensor(b!) seqused_k, Tensor block_table, Tensor? kv_new, "
  "Tensor? cache_seqlens, int max_seqlen_q, int max_seqlen_k, float softmax_scale, int causal, int num_splits=0) -> (Tensor o, Tensor softmax_lse)",
)


@torch.library.impl(f"{_OP_NAMESPACE}::_mla_fp8_fwd_hip", "CUDA")  # ROCm tensors dispatch on the CUDA key
def _mla_fp8_fwd_hip_torch_op(q, kv_cache, head_dim_v, kv_scale, cu_seqlens_q, seqused_k, block_table, kv_new, cache_seqlens, max_seqlen_q, max_seqlen_k,
                              softmax_scale, causal, num_splits=0):
  return mla_fp8_forward(q, kv_cache, int(head_dim_v), cu_seqlens_q, seqused_k, block_table, max_seqlen_q, max_seqlen_k, bool(causal), softmax_scale, kv_scale,
                         kv_new=kv_new, cache_seqlens=cache_seqlens, return_lse=True, num_splits=num_splits)


torch.library.register_fake(f"{_OP_NAMESPACE}::_mla_fp8_fwd_hip", _mla_out_fake)


# The tree-mask latent call (ffpa_attn_with_kvcache_mla_tree / ffpa_attn_varlen_with_kvcache_mla_tree): the latent call's op with the mask words — kv_cache is written
# in place by the append (kv_new), as there; nothing else is marked written
torch.library.define(
  f"{_OP_NAMESPACE}::_mla_tree_fwd_hip",
  "(Tensor q, Tensor(a!) kv_cache, int head_dim_v, Tensor cu_seqlens_q, Tensor(b!) seqused_k, Tensor block_table, Tensor tree_words, Tensor? kv_new, "
  "Tensor? cache_seqlens, int max_seqlen_q, int max_seqlen_k, float softmax_scale, int num_splits=0) -> (Tensor o, Tensor softmax_lse)",
)


@torch.library.impl(f"{_OP_NAMESPACE}::_mla_tree_fwd_hip", "CUDA")  # ROCm tensors dispatch on the CUDA key
def _mla_tree_fwd_hip_torch_op(q, kv_cache, head_dim_v, cu_seqlens_q, seqused_k, block_table, tree_words, kv_new, cache_seqlens, max_seqlen_q, max_seqlen_k,
                               softmax_scale, num_splits=0):
  return mla_tree_forward(q, kv_cache, int(head_dim_v), cu_seqlens_q, seqused_k, block_table, max_seqlen_q, max_seqlen_k, softmax_scale, tree_words, kv_new=kv_new,
                          cache_seqlens=cache_seqlens, return_lse=True, num_splits=num_splits)


torch.library.register_fake(f"{_OP_NAMESPACE}::_mla_tree_fwd_hip", _mla_out_fake)


# The tree-mask latent call over an FP8 pool (ffpa_attn_with_kvcache_mla_tree_fp8 / ffpa_attn_varlen_with_kvcache_mla_tree_fp8): the tree op with the per-tensor scale —
# kv_cache (float8_e4m3fn) is written in place by the quantising append (kv_new)
torch.library.define(
  f"{_OP_NAMESPACE}::_mla_tree_fp8_fwd_hip",
  "(Tensor q, Tensor(a!) kv_cache, int head_dim_v, float kv_scale, Tensor cu_seqlens_q, Tensor(b!) seqused_k, Tensor block_table, Tensor tree_words, "
  "Tensor? kv_new, Tensor? cache_seqlens, int max_seqlen_q, int max_seqlen_k, float softmax_scale, int num_splits=0) -> (Tensor o, Tensor softmax_lse)",
)


@torch.library.impl(f"{_OP_NAMESPACE}::_mla_tree_fp8_fwd_hip", "CUDA")  # ROCm tensors dispatch on the CUDA key
def _mla_tree_fp8_fwd_hip_torch_op(q, kv_cache, head_dim_v, kv_scale, cu_seqlens_q, seqused_k, block_table, tree_words, kv_new, cache_seqlens, max_seqlen_q,
                                   max_seqlen_k, softmax_scale, num_splits=0):
  return mla_tree_fp8_forward(q, kv_cache, int(head_dim_v), cu_seqlens_q, seqused_k, block_table, max_seqlen_q, max_seqlen_k, softmax_scale, tree_words, kv_scale,
                              kv_new=kv_new, cache_seqlens=cache_seqlens, return_lse=True, num_splits=num_splits)


torch.library.register_fake(f"{_OP_NAMESPACE}::_mla_tree_fp8_fwd_hip", _mla_out_fake)


# The sparse latent call (ffpa_attn_with_kvcache_mla_sparse): every query token attends to the latent rows its index list names
MLA_SPARSE_SPAN_BYTES = 1 << 31  # what the kernel's 32-bit lane offsets reach: a head's rows of the pool span at most this many bytes (bit 31 = "no row")
_MLA_SPARSE_IDENTITY: "dict[tuple, torch.Tensor]" = {}


def mla_sparse_pool(kv_cache: torch.Tensor, name: str = "ffpa_attn::_mla_sparse_fwd_hip") -> "tuple[int, int, int]":
  """``(num_rows, row stride, head stride)`` — elements — of a latent pool as the sparse call addresses it: the flat ``[num_rows, Hkv, D]``, or a page pool
  ``[num_pages, page_size, Hkv, D]`` of any positive ``page_size`` whose pages are evenly spaced (slot r = row ``r % page_size`` of page ``r // page_size`` then
  lies ``r`` row strides from the base).  ``ValueError``: pages that are not evenly spaced, and a pool whose rows span more than ``MLA_SPARSE_SPAN_BYTES`` —
  from sizes and strides alone, so in front of any launch and without touching the pool's memory."""
  num_rows, row_stride, head_stride = _mla_sparse_slots(kv_cache, name)
  if kv_cache.element_size() == 1 and (row_stride % 16 != 0 or head_stride % 16 != 0):
    # (an FP8 pool: its loads are 8 bytes wide and the kernel's text doubles every stride; the span below counts its bytes — twice the rows of a 16-bit pool)
    raise ValueError(f"{name}: the row and head strides of an FP8 pool ({row_stride}, {head_stride}) must be multiples of 16 elements")
  span = (num_rows - 1) * row_stride * kv_cache.element_size() + kv_cache.size(-1) * kv_cache.element_size() if num_rows > 0 else 0
  if span > MLA_SPARSE_SPAN_BYTES:
    raise ValueError(f"{name}: the pool's rows span {span} bytes per latent head ((num_rows - 1) * row stride + one row = ({num_rows} - 1) * "
                     f"{row_stride * kv_cache.element_size()} + {kv_cache.size(-1) * kv_cache.element_size()}); the sparse call's 32-bit offsets reach at most "
                     f"2^31 = {MLA_SPARSE_SPAN_BYTES} bytes: hand it a view of the part of the pool the step's slots lie in")
  return num_rows, row_stride, head_stride


def _mla_sparse_slots(kv_cache: torch.Tensor, name: str) -> "tuple[int, int, int]":
  """``mla_sparse_pool``'s first half, shared with ``mla_sparse_ds_pool``: the two pool forms -> ``(num_rows, row stride, head stride)`` in elements."""
  if kv_cache.dim() == 4:
    pages, page_size = kv_cache.size(0), kv_cache.size(1)
    if page_size <= 0:
      raise ValueError(f"{name}: page_size ({page_size}) must be positive")
    if pages > 1 and page_size > 1 and kv_cache.stride(0) != page_size * kv_cache.stride(1):
      raise ValueError(f"{name}: the pages of kv_cache must be evenly spaced — stride(0) == page_size * stride(1), got {kv_cache.stride(0)} and "
                       f"{page_size} * {kv_cache.stride(1)}: slot r must lie r rows from the pool's base")
    num_rows, row_stride, head_stride = pages * page_size, kv_cache.stride(1) if page_size > 1 else kv_cache.stride(0), kv_cache.stride(2)
  elif kv_cache.dim() == 3:
    num_rows, row_stride, head_stride = kv_cache.size(0), kv_cache.stride(0), kv_cache.stride(1)
  else:
    raise ValueError(f"{name}: kv_cache must be the flat pool [num_rows, Hkv, D] or a page pool [num_pages, page_size, Hkv, D], got {kv_cache.dim()}-D")
  if num_rows > 0x7fffffff:
    raise ValueError(f"{name}: a pool of {num_rows} rows is too large (slots are int32)")
  return num_rows, row_stride, head_stride


MLA_DS_ROW_BYTES = 656  # a latent row of DeepSeek-V3.2's FP8 cache: 512 e4m3 codes, four float32 scales (one per 128 columns), 64 bf16 rotary columns


def mla_sparse_ds_pool(kv_cache: torch.Tensor, name: str = "ffpa_attn::_mla_sparse_ds_fwd_hip") -> "tuple[int, int, int]":
  """``mla_sparse_pool`` for a ``torch.uint8`` pool of 656-byte rows -> ``(num_rows, slot stride, head stride)`` in BYTES.  ``ValueError``: pages that are not
  evenly spaced, a stride that is no multiple of 16 or a slot stride below 656, a pool whose rows span more than ``MLA_SPARSE_SPAN_BYTES``."""
  num_rows, row_stride, head_stride = _mla_sparse_slots(kv_cache, name)
  if row_stride % 16 != 0 or head_stride % 16 != 0 or (num_rows > 1 and row_stride < MLA_DS_ROW_BYTES):
    raise ValueError(f"{name}: the slot and head strides of the pool ({row_stride}, {head_stride}) must be multiples of 16 bytes, slots at least "
                     f"{MLA_DS_ROW_BYTES} bytes apart")
  span = (num_rows - 1) * row_stride + MLA_DS_ROW_BYTES if num_rows > 0 else 0
  if span > MLA_SPARSE_SPAN_BYTES:
    raise ValueError(f"{name}: the pool's rows span {span} bytes per latent head ((num_rows - 1) * slot stride + one row = ({num_rows} - 1) * {row_stride} + "
                     f"{MLA_DS_ROW_BYTES}); the sparse call's 32-bit offsets reach at most 2^31 = {MLA_SPARSE_SPAN_BYTES} bytes: hand it a view of the part of "
                     "the pool the step's slots lie in")
  return num_rows, row_stride, head_stride


def _mla_sparse_cu_q(T: int, device) -> torch.Tensor:
  """The boundaries of T one-token sequences, 0 ... T, made on the device once per (T, device)."""
  key = (T, device.type, device.index)
  t = _MLA_SPARSE_IDENTITY.get(key)
  if t is None and torch.cuda.is_current_stream_capturing():
    return torch.arange(T + 1, dtype=torch.int32, device=device)  # (memory of the graph's own pool: not kept for calls outside the graph)
  if t is None:
    if len(_MLA_SPARSE_IDENTITY) >= 64:
      _MLA_SPARSE_IDENTITY.clear()
    t = _MLA_SPARSE_IDENTITY[key] = torch.arange(T + 1, dtype=torch.int32, device=device)
  return t


def _mla_sparse_args(dtype, T: int, Hq: int, Hkv: int, D: int, head_dim_v: int, topk: int, num_rows: int, row_stride: int, head_stride: int, q_strides, o_strides,
                     softmax_scale: float, flags: int, num_splits: int, indices_stride: "int | None" = None):
  """``(ffpa_varlen_fwd_params, ffpa_mla_sparse)`` of the sparse call without their pointers: the shape class, the strides and the scalars."""
  p = _varlen_params(dtype, T, Hq, Hkv, D, 1, topk, T, [q_strides, (row_stride, head_stride), (row_stride, head_stride), o_strides], False, softmax_scale, -1.0,
                     flags, num_splits)
  s = _stamped(FfpaMlaSparse)
  s.indices_stride = topk if indices_stride is None else indices_stride
  s.kv_stride[:] = [row_stride, head_stride]
  s.topk, s.num_rows, s.head_dim_v = topk, num_rows, int(head_dim_v)
  return p, s


def mla_sparse_forward(q: torch.Tensor, kv_cache: torch.Tensor, head_dim_v: int, indices: torch.Tensor, topk_lens: "torch.Tensor | None", softmax_scale: float, *,
                       return_lse: bool = True, flags: int = 0, plan_out: "dict | None" = None, num_splits: int = 0, kv_scale: "float | None" = None,
                       ds: bool = False):
  """One call of ``ffpa_attn_varlen_mla_sparse_fwd``: ``q [T, Hq, D]`` (one row per query token), the latent pool ``kv_cache`` (``mla_sparse_pool``'s two forms),
  the int32 device ``indices [T, topk]`` of pool slots and the optional int32 ``topk_lens [T]`` -> ``(o [T, Hq, head_dim_v], lse [Hq, T] fp32 | None)``.  Token t
  attends to the rows ``indices[t, :clamp(topk_lens[t], 0, topk)]``; entries at and past the count are never turned into an address.  Nothing is read back to the
  host: the call (and the split launch's merge) captures into a HIP graph.  ``flags`` / ``plan_out`` / ``num_splits`` as ``varlen_forward``.

  ``kv_scale`` (a host float, finite and > 0; ``mla_sparse_fp8_forward`` is this call with it): the pool is ``torch.float8_e4m3fn`` — OCP e4m3 codes, K = kv_scale x
  K8, row and head strides multiples of 16 — and the call is ``ffpa_attn_varlen_mla_sparse_fp8_fwd``, its own kernel; q and o stay bf16 / fp16.

  ``ds`` (``mla_sparse_ds_forward`` is this call with it): the pool is ``torch.uint8`` rows of ``MLA_DS_ROW_BYTES`` (``mla_sparse_ds_pool``'s two forms, strides in
  bytes), q and o are bf16, and the call is ``ffpa_attn_varlen_mla_sparse_ds_fwd``."""
  fp8 = kv_scale is not None
  name = "ffpa_attn::_mla_sparse_ds_fwd_hip" if ds else "ffpa_attn::_mla_sparse_fp8_fwd_hip" if fp8 else "ffpa_attn::_mla_sparse_fwd_hip"
  export = "ffpa_attn_varlen_mla_sparse_ds_fwd" if ds else "ffpa_attn_varlen_mla_sparse_fp8_fwd" if fp8 else "ffpa_attn_varlen_mla_sparse_fwd"
  if not q.is_cuda:
    raise NotImplementedError(f"{name} has no implementation for device '{q.device.type}' (the HIP kernel needs a GPU tensor)")
  lib = load_library()
  if ds:
    if q.dtype != torch.bfloat16 or kv_cache.dtype != torch.uint8:
      raise TypeError(f"{name} only supports bf16 q over a torch.uint8 kv_cache of {MLA_DS_ROW_BYTES}-byte rows, got {q.dtype}, {kv_cache.dtype}")
  elif fp8:
    if q.dtype not in _DTYPE or kv_cache.dtype != torch.float8_e4m3fn:
      raise TypeError(f"{name} only supports fp16/bf16 q over a torch.float8_e4m3fn kv_cache (OCP e4m3, the chip's FP8 format), got {q.dtype}, {kv_cache.dtype}")
    kv_scale = check_kv_scale(kv_scale, name)
  elif q.dtype not in _DTYPE or kv_cache.dtype != q.dtype:
    raise TypeError(f"{name} only supports fp16/bf16 q/kv_cache of one dtype, got {q.dtype}, {kv_cache.dtype}")
  if q.dim() != 3 or kv_cache.dim() not in (3, 4) or kv_cache.size(-1) != (MLA_DS_ROW_BYTES if ds else q.size(2)):
    raise ValueError(f"{name}: q must be [T, Hq, D] and kv_cache [num_rows, Hkv, D] or [num_pages, page_size, Hkv, D] of " +
                     (f"{MLA_DS_ROW_BYTES}-byte rows" if ds else "q's head dim"))
  T, Hq, D = q.shape
  Hkv = kv_cache.size(-2)
  if (D, int(head_dim_v)) not in MLA_BUILDS:
    raise NotImplementedError(f"{name}: (head_dim, head_dim_v) = ({D}, {head_dim_v}) is not built (built: {', '.join(map(str, MLA_BUILDS))})")
  if Hkv == 0 or Hq % Hkv != 0:
    raise ValueError(f"{name}: query num_heads ({Hq}) must be a multiple of the latent num_heads ({Hkv})")
  if indices.dtype != torch.int32 or indices.dim() != 2 or indices.size(0) != T or indices.size(1) < 1 or indices.device != q.device:
    raise ValueError(f"{name}: indices must be a 2-D int32 tensor [T={T}, topk >= 1] on q's device")
  if topk_lens is not None and (topk_lens.dtype != torch.int32 or topk_lens.dim() != 1 or topk_lens.numel() != T or topk_lens.device != q.device):
    raise ValueError(f"{name}: topk_lens must be a 1-D int32 tensor of length T={T} on q's device")
  if kv_cache.device != q.device or kv_cache.numel() == 0:
    raise ValueError(f"{name}: kv_cache must be a non-empty pool on q's device")
  if not _layout_ok(kv_cache, -3):
    raise ValueError(f"{name}: kv_cache needs head-dim stride 1, strides that are multiples of {16 if fp8 or ds else 8} elements and a 16-byte aligned base (it is "
                     "read in place)")
  num_rows, row_stride, head_stride = (mla_sparse_ds_pool if ds else mla_sparse_pool)(kv_cache, name)
  topk = indices.size(1)
  q = _rows(q, 0)
  if indices.stride(1) != 1 or indices.data_ptr() % 4 != 0 or (T > 1 and indices.stride(0) < topk):
    indices = indices.contiguous()
  if topk_lens is not None and not topk_lens.is_contiguous():
    topk_lens = topk_lens.contiguous()
  o = torch.empty((T, Hq, int(head_dim_v)), dtype=q.dtype, device=q.device)
  lse = torch.empty((Hq, T), dtype=torch.float32, device=q.device) if return_lse else None
  if T == 0:
    return o, lse
  p, s = _mla_sparse_args(q.dtype, T, Hq, Hkv, D, head_dim_v, topk, num_rows, row_stride, head_stride, q.stride()[-3:-1], o.stride()[-3:-1], softmax_scale,
                          int(flags) | _deterministic_flag(), num_splits, indices.stride(0) if T > 1 else topk)
  cu_q = _mla_sparse_cu_q(T, q.device)
  p.q, p.k, p.v, p.o = q.data_ptr(), kv_cache.data_ptr(), kv_cache.data_ptr(), o.data_ptr()
  p.lse = lse.data_ptr() if lse is not None else None
  p.lse_stride_head = lse.stride(0) if lse is not None else 0
  p.cu_seqlens_q = cu_q.data_ptr()
  s.indices = indices.data_ptr()
  s.topk_lens = topk_lens.data_ptr() if topk_lens is not None else None
  args = (ctypes.byref(p), ctypes.byref(s))
  if fp8:
    f8 = _stamped(FfpaMlaFp8)
    f8.kv_scale = kv_scale
    args += (ctypes.byref(f8),)
  with torch.cuda.device(q.device):
    stream = torch.cuda.current_stream(q.device).cuda_stream
    nbytes = 0
    if not (p.num_splits == 1 or p.flags & FLAG_DETERMINISTIC):
      key = ("sparse", id(lib), q.device.index or 0, p.dtype, T, Hq, Hkv, D, s.head_dim_v, topk, p.flags, p.num_splits, os.environ.get("FFPA_HIP_FAKE_CUS")) + (
        ("ds",) if ds else ("fp8",) if fp8 else ())
      nbytes = _cached_scratch(_MLA_SCRATCH, key, lambda: int(getattr(lib, export + "_workspace_bytes")(*args)))
    workspace = _hand_over_workspace(p, q.device, stream, nbytes)  # (held in a local until the launch below has been enqueued)
    if plan_out is not None:
      plan_out.update(_read_plan(lib, getattr(lib, export + "_plan"), getattr(lib, export + "_kernel"), _VARLEN_PLAN_KEYS, args))
    rc = getattr(lib, export)(*args, ctypes.c_void_p(stream))
  if rc != 0:
    _raise_status(lib, rc, export)
  return o, lse


def mla_sparse_fp8_forward(q: torch.Tensor, kv_cache: torch.Tensor, head_dim_v: int, indices: torch.Tensor, topk_lens: "torch.Tensor | None", softmax_scale: float,
                           kv_scale: float, *, return_lse: bool = True, flags: int = 0, plan_out: "dict | None" = None, num_splits: int = 0):
  """One call of ``ffpa_attn_varlen_mla_sparse_fp8_fwd`` — the sparse latent call over a ``torch.float8_e4m3fn`` pool with the per-tensor ``kv_scale``
  (``mla_sparse_forward``'s ``kv_scale``).  ``flags`` / ``plan_out`` / ``num_splits`` as there (tests force or inspect the launch)."""
  if kv_scale is None:
    raise ValueError("ffpa_attn::_mla_sparse_fp8_fwd_hip: kv_scale is required")
  return mla_sparse_forward(q, kv_cache, head_dim_v, indices, topk_lens, softmax_scale, return_lse=return_lse, flags=flags, plan_out=plan_out, num_splits=num_splits,
                            kv_scale=kv_scale)


torch.library.define(
  f"{_OP_NAMESPACE}::_mla_sparse_fwd_hip",
  "(Tensor q, Tensor kv_cache, int head_dim_v, Tensor indices, Tensor? topk_lens, float softmax_scale, int num_splits=0) -> (Tensor o, Tensor softmax_lse)",
)


@torch.library.impl(f"{_OP_NAMESPACE}::_mla_sparse_fwd_hip", "CUDA")  # ROCm tensors dispatch on the CUDA key
def _mla_sparse_fwd_hip_torch_op(q, kv_cache, head_dim_v, indices, topk_lens, softmax_scale, num_splits=0):
  return mla_sparse_forward(q, kv_cache, int(head_dim_v), indices, topk_lens, softmax_scale, return_lse=True, num_splits=num_splits)


torch.library.register_fake(f"{_OP_NAMESPACE}::_mla_sparse_fwd_hip", _mla_out_fake)


# The sparse latent call over an FP8 pool (ffpa_attn_with_kvcache_mla_sparse_fp8): the sparse op with the per-tensor scale
torch.library.define(
  f"{_OP_NAMESPACE}::_mla_sparse_fp8_fwd_hip",
  "(Tensor q, Tensor kv_cache, int head_dim_v, float kv_scale, Tensor indices, Tensor? topk_lens, float softmax_scale, int num_splits=0) -> "
  "(Tensor o, Tensor softmax_lse)",
)


@torch.library.impl(f"{_OP_NAMESPACE}::_mla_sparse_fp8_fwd_hip", "CUDA")  # ROCm tensors dispatch on the CUDA key
def _mla_sparse_fp8_fwd_hip_torch_op(q, kv_cache, head_dim_v, kv_scale, indices, topk_lens, softmax_scale, num_splits=0):
  return mla_sparse_fp8_forward(q, kv_cache, int(head_dim_v), indices, topk_lens, softmax_scale, kv_scale, return_lse=True, num_splits=num_splits)


torch.library.register_fake(f"{_OP_NAMESPACE}::_mla_sparse_fp8_fwd_hip", _mla_out_fake)


# The sparse latent call over DeepSeek-V3.2's 656-byte FP8 rows (ffpa_attn_with_kvcache_mla_sparse_ds): the sparse op over a uint8 pool — and the store that writes
# such rows by slot (store_latent_rows_ds), which mutates the pool
def mla_sparse_ds_forward(q: torch.Tensor, kv_cache: torch.Tensor, head_dim_v: int, indices: torch.Tensor, topk_lens: "torch.Tensor | None", softmax_scale: float, *,
                          return_lse: bool = True, flags: int = 0, plan_out: "dict | None" = None, num_splits: int = 0):
  """One call of ``ffpa_attn_varlen_mla_sparse_ds_fwd`` — the sparse latent call over a ``torch.uint8`` pool of 656-byte rows (``mla_sparse_forward``'s ``ds``).
  ``flags`` / ``plan_out`` / ``num_splits`` as there (tests force or inspect the launch)."""
  return mla_sparse_forward(q, kv_cache, head_dim_v, indices, topk_lens, softmax_scale, return_lse=return_lse, flags=flags, plan_out=plan_out, num_splits=num_splits,
                            ds=True)


torch.library.define(
  f"{_OP_NAMESPACE}::_mla_sparse_ds_fwd_hip",
  "(Tensor q, Tensor kv_cache, int head_dim_v, Tensor indices, Tensor? topk_lens, float softmax_scale, int num_splits=0) -> (Tensor o, Tensor softmax_lse)",
)


@torch.library.impl(f"{_OP_NAMESPACE}::_mla_sparse_ds_fwd_hip", "CUDA")  # ROCm tensors dispatch on the CUDA key
def _mla_sparse_ds_fwd_hip_torch_op(q, kv_cache, head_dim_v, indices, topk_lens, softmax_scale, num_splits=0):
  return mla_sparse_ds_forward(q, kv_cache, int(head_dim_v), indices, topk_lens, softmax_scale, return_lse=True, num_splits=num_splits)


torch.library.register_fake(f"{_OP_NAMESPACE}::_mla_sparse_ds_fwd_hip", _mla_out_fake)


def mla_ds_store(kv_cache: torch.Tensor, kv_new: torch.Tensor, slots: torch.Tensor) -> None:
  """One launch of ``ffpa_attn_mla_ds_store``: row t of the bf16 ``kv_new [T, Hkv, 576]`` is packed (``pack_latent_rows_ds``, to the byte) into slot ``slots[t]``
  of the ``torch.uint8`` pool ``kv_cache`` (``mla_sparse_ds_pool``'s two forms), in place.  ``slots``: int32 ``[T]`` on the device; a slot < 0 or >= the pool's
  rows writes nothing.  Asynchronous, nothing read back to the host."""
  name = "ffpa_attn::_mla_ds_store_hip"
  if not kv_cache.is_cuda:
    raise NotImplementedError(f"{name} has no implementation for device '{kv_cache.device.type}' (the HIP kernel needs a GPU tensor)")
  lib = load_library()
  if kv_new.dtype != torch.bfloat16 or kv_cache.dtype != torch.uint8:
    raise TypeError(f"{name} only supports bf16 kv over a torch.uint8 kv_cache of {MLA_DS_ROW_BYTES}-byte rows, got {kv_new.dtype}, {kv_cache.dtype}")
  if kv_new.dim() != 3 or kv_cache.dim() not in (3, 4) or kv_cache.size(-1) != MLA_DS_ROW_BYTES or kv_new.size(1) != kv_cache.size(-2):
    raise ValueError(f"{name}: kv must be [T, Hkv, D] and kv_cache [num_rows, Hkv, {MLA_DS_ROW_BYTES}] or [num_pages, page_size, Hkv, {MLA_DS_ROW_BYTES}] of the "
                     "same Hkv")
  T, Hkv, D = kv_new.shape
  if (D, 512) not in MLA_BUILDS:
    raise NotImplementedError(f"{name}: rows of {D} columns are not built (built: 576 = 512 quantised + 64 rotary)")
  if slots.dtype != torch.int32 or slots.dim() != 1 or slots.numel() != T or slots.device != kv_cache.device or kv_new.device != kv_cache.device:
    raise ValueError(f"{name}: slots must be an int32 tensor [T={T}] and kv, slots and kv_cache on one device")
  if not _layout_ok(kv_cache, -3) or kv_cache.numel() == 0:
    raise ValueError(f"{name}: kv_cache needs a non-empty pool with unit stride in the last dimension, strides that are multiples of 16 bytes and a 16-byte "
                     "aligned base (it is written in place)")
  num_rows, row_stride, head_stride = mla_sparse_ds_pool(kv_cache, name)
  if T == 0:
    return
  kv_new = _rows(kv_new, 0)
  if not slots.is_contiguous():
    slots = slots.contiguous()
  p = _stamped(FfpaMlaDsStoreParams)
  p.kv_new, p.slots, p.kv_cache = kv_new.data_ptr(), slots.data_ptr(), kv_cache.data_ptr()
  p.kv_new_stride[:] = list(kv_new.stride()[:2])
  p.kv_cache_stride[:] = [row_stride, head_stride]
  p.tokens, p.heads_kv, p.num_rows, p.head_dim, p.dtype = T, Hkv, num_rows, D, _DTYPE[kv_new.dtype]
  with torch.cuda.device(kv_cache.device):
    rc = lib.ffpa_attn_mla_ds_store(ctypes.byref(p), ctypes.c_void_p(torch.cuda.current_stream(kv_cache.device).cuda_stream))
  if rc != 0:
    _raise_status(lib, rc, "ffpa_attn_mla_ds_store")


torch.library.define(f"{_OP_NAMESPACE}::_mla_ds_store_hip", "(Tensor(a!) kv_cache, Tensor kv_new, Tensor slots) -> ()")


@torch.library.impl(f"{_OP_NAMESPACE}::_mla_ds_store_hip", "CUDA")  # ROCm tensors dispatch on the CUDA key
def _mla_ds_store_hip_torch_op(kv_cache, kv_new, slots):
  mla_ds_store(kv_cache, kv_new, slots)


@torch.library.register_fake(f"{_OP_NAMESPACE}::_mla_ds_store_hip")
def _mla_ds_store_fake(kv_cache, kv_new, slots):
  return None


# The launch that makes the sparse latent calls' inputs (ffpa_mla_sparse_topk_slots / ffpa_mla_sparse_slots, ffpa_attn_amd/kvcache.py, where the arguments are checked)
def mla_sparse_topk(rows: torch.Tensor, by_score: bool, topk: int, cache_seqlens: torch.Tensor, block_table: "torch.Tensor | None", page_size: int,
                    cu_seqlens_q: "torch.Tensor | None", causal: bool) -> "tuple[torch.Tensor, torch.Tensor]":
  """One launch of ``ffpa_attn_mla_sparse_topk_slots``: ``rows`` is the float32 ``scores [T, N]`` (``by_score``) or the int32 ``positions [T, topk]`` ->
  ``(indices int32 [T, topk], topk_lens int32 [T])`` on the device.  Asynchronous, nothing read back to the host."""
  name = "ffpa_attn::_mla_sparse_topk_slots_hip" if by_score else "ffpa_attn::_mla_sparse_slots_hip"
  if not rows.is_cuda:
    raise NotImplementedError(f"{name} has no implementation for device '{rows.device.type}' (the HIP kernel needs a GPU tensor)")
  lib = load_library()
  T = rows.size(0)
  indices = torch.empty((T, topk), dtype=torch.int32, device=rows.device)
  topk_lens = torch.empty((T,), dtype=torch.int32, device=rows.device)
  if T == 0:
    return indices, topk_lens
  cache_seqlens = cache_seqlens.contiguous()
  p = _stamped(FfpaMlaSparseTopkParams)
  if by_score:
    p.scores = rows.data_ptr()
  else:
    p.positions = rows.data_ptr()
  p.cache_seqlens, p.indices, p.topk_lens = cache_seqlens.data_ptr(), indices.data_ptr(), topk_lens.data_ptr()
  if cu_seqlens_q is not None:
    cu_seqlens_q = cu_seqlens_q.contiguous()
    p.cu_seqlens_q = cu_seqlens_q.data_ptr()
  if block_table is not None:
    p.block_table, p.block_table_stride, p.W, p.page_size = block_table.data_ptr(), block_table.stride(0), block_table.size(1), page_size
  p.row_stride, p.indices_stride = rows.stride(0), topk
  p.T, p.N_or_topk, p.topk, p.B, p.causal = T, rows.size(1), topk, cache_seqlens.numel(), int(bool(causal))
  rc = _call_on_stream(lib.ffpa_attn_mla_sparse_topk_slots, rows.device, ctypes.byref(p))
  if rc != 0:
    _raise_status(lib, rc, "ffpa_attn_mla_sparse_topk_slots")
  return indices, topk_lens


torch.library.define(
  f"{_OP_NAMESPACE}::_mla_sparse_topk_slots_hip",
  "(Tensor scores, int topk, Tensor cache_seqlens, Tensor? block_table, int page_size, Tensor? cu_seqlens_q, bool causal) -> (Tensor indices, Tensor topk_lens)",
)
torch.library.define(
  f"{_OP_NAMESPACE}::_mla_sparse_slots_hip",
  "(Tensor positions, Tensor cache_seqlens, Tensor? block_table, int page_size, Tensor? cu_seqlens_q) -> (Tensor indices, Tensor topk_lens)",
)


@torch.library.impl(f"{_OP_NAMESPACE}::_mla_sparse_topk_slots_hip", "CUDA")  # ROCm tensors dispatch on the CUDA key
def _mla_sparse_topk_slots_hip_torch_op(scores, topk, cache_seqlens, block_table, page_size, cu_seqlens_q, causal):
  return mla_sparse_topk(scores, True, int(topk), cache_seqlens, block_table, int(page_size), cu_seqlens_q, causal)


@torch.library.impl(f"{_OP_NAMESPACE}::_mla_sparse_slots_hip", "CUDA")
def _mla_sparse_slots_hip_torch_op(positions, cache_seqlens, block_table, page_size, cu_seqlens_q):
  return mla_sparse_topk(positions, False, positions.size(1), cache_seqlens, block_table, int(page_size), cu_seqlens_q, False)


@torch.library.register_fake(f"{_OP_NAMESPACE}::_mla_sparse_topk_slots_hip")
def _mla_sparse_topk_slots_fake(scores, topk, cache_seqlens, block_table, page_size, cu_seqlens_q, causal):
  return scores.new_empty((scores.size(0), topk), dtype=torch.int32), scores.new_empty((scores.size(0),), dtype=torch.int32)


@torch.library.register_fake(f"{_OP_NAMESPACE}::_mla_sparse_slots_hip")
def _mla_sparse_slots_fake(positions, cache_seqlens, block_table, page_size, cu_seqlens_q):
  return torch.empty_like(positions, memory_format=torch.contiguous_format), positions.new_empty((positions.size(0),))


# The latent append of a ragged step (ffpa_attn_varlen_with_kvcache_mla(kv=)): token rows packed by cu_seqlens_q, in front of the attention launch
def mla_append_varlen(kv_cache: torch.Tensor, kv_new: torch.Tensor, cu_seqlens_q: torch.Tensor, cache_seqlens: torch.Tensor, block_table: torch.Tensor,
                      kv_scale: "float | None" = None) -> torch.Tensor:
  """One launch of ``ffpa_attn_mla_append_varlen``: ``kv_new [T, Hkv, D]``, packed by the int32 device ``cu_seqlens_q [B + 1]``, written into the latent pool
  ``kv_cache [num_pages, page_size, Hkv, D]`` in place through the int32 ``block_table [B, pages_per_seq]`` — token i of sequence b at cache position
  ``max(cache_seqlens[b], 0) + i``, every element stored once, positions at or past the capacity dropped, rows at or past ``cu_seqlens_q[B]`` not written
  -> ``seqused``: the int32 ``[B]`` post-append lengths ``min(max(cache_seqlens, 0) + Sq_b, capacity)``, sequences without a token included.  Asynchronous,
  nothing read back to the host.  ``kv_scale`` (a host float): the pool is ``torch.float8_e4m3fn`` and the launch is ``ffpa_attn_mla_fp8_append_varlen`` — the
  bf16 / fp16 rows of ``kv_new`` are stored as ``quantize_latent_rows(kv_new, kv_scale)``."""
  fp8 = kv_scale is not None
  name = "ffpa_attn::_mla_fp8_append_varlen_hip" if fp8 else "ffpa_attn::_mla_append_varlen_hip"
  if not kv_cache.is_cuda:
    raise NotImplementedError(f"{name} has no implementation for device '{kv_cache.device.type}' (the HIP kernel needs a GPU tensor)")
  lib = load_library()
  if fp8:
    if kv_new.dtype not in _DTYPE or kv_cache.dtype != torch.float8_e4m3fn:
      raise TypeError(f"{name} only supports fp16/bf16 kv_new into a torch.float8_e4m3fn kv_cache (OCP e4m3), got {kv_new.dtype}, {kv_cache.dtype}")
    kv_scale = check_kv_scale(kv_scale, name)
  elif kv_cache.dtype not in _DTYPE or kv_new.dtype != kv_cache.dtype:
    raise TypeError(f"{name} only supports fp16/bf16 kv_cache/kv_new of one dtype, got {kv_cache.dtype}, {kv_new.dtype}")
  if kv_cache.dim() != 4 or kv_new.dim() != 3 or tuple(kv_new.shape[1:]) != tuple(kv_cache.shape[2:]):
    raise ValueError(f"{name}: kv_new must be [T, Hkv={kv_cache.size(2)}, D={kv_cache.size(3)}] for the pool {tuple(kv_cache.shape)}, got {tuple(kv_new.shape)}")
  if cu_seqlens_q.dtype != torch.int32 or cu_seqlens_q.dim() != 1 or cu_seqlens_q.numel() < 2 or cu_seqlens_q.device != kv_cache.device:
    raise ValueError(f"{name}: cu_seqlens_q must be a 1-D int32 tensor of length batch + 1 on the cache's device")
  B = cu_seqlens_q.numel() - 1
  if cache_seqlens.dtype != torch.int32 or cache_seqlens.dim() != 1 or cache_seqlens.numel() != B or cache_seqlens.device != kv_cache.device:
    raise ValueError(f"{name}: cache_seqlens must be a 1-D int32 tensor of length batch on the cache's device")
  if block_table.dtype != torch.int32 or block_table.dim() != 2 or block_table.size(0) != B or block_table.size(1) == 0 or block_table.device != kv_cache.device:
    raise ValueError(f"{name}: block_table must be a 2-D int32 tensor [batch, pages_per_seq] (pages_per_seq >= 1) on the cache's device")
  if kv_new.device != kv_cache.device or kv_cache.size(0) == 0:
    raise ValueError(f"{name}: kv_new and a non-empty kv_cache must be on one device")
  if not _layout_ok(kv_cache, -3) or (fp8 and any(st % 16 for st in kv_cache.stride()[:-1])):
    raise ValueError(f"{name}: kv_cache is written in place and needs head-dim stride 1, strides that are multiples of {16 if fp8 else 8} elements and a 16-byte aligned base")
  kv_new = _rows(kv_new)
  cache_seqlens, cu_seqlens_q = cache_seqlens.contiguous(), cu_seqlens_q.contiguous()
  seqused = torch.empty((B,), dtype=torch.int32, device=kv_cache.device)
  p = _stamped(FfpaMlaAppendVarlenParams)
  p.kv_cache = kv_cache.data_ptr()
  p.cu_seqlens_q, p.cache_seqlens, p.seqused = cu_seqlens_q.data_ptr(), cache_seqlens.data_ptr(), seqused.data_ptr()
  p.kv_cache_stride[:] = list(kv_cache.stride()[-3:-1])
  p.batch, p.total_q, p.heads_kv, p.head_dim, p.dtype = B, kv_new.size(0), kv_cache.size(2), kv_cache.size(3), _DTYPE[kv_new.dtype]
  if kv_new.size(0) > 0:
    p.kv_new = kv_new.data_ptr()
    p.kv_new_stride[:] = list(kv_new.stride()[:2])
  kv, block_table = _paged_kv_of(block_table, kv_cache, kv_cache)
  if fp8:
    f8 = _stamped(FfpaMlaFp8)
    f8.kv_scale = kv_scale
    rc = _call_on_stream(lib.ffpa_attn_mla_fp8_append_varlen, kv_cache.device, ctypes.byref(p), ctypes.byref(kv), ctypes.byref(f8))
  else:
    rc = _call_on_stream(lib.ffpa_attn_mla_append_varlen, kv_cache.device, ctypes.byref(p), ctypes.byref(kv))
  if rc != 0:
    _raise_status(lib, rc, "ffpa_attn_mla_fp8_append_varlen" if fp8 else "ffpa_attn_mla_append_varlen")
  return seqused


# kv_cache is written in place: the schema says so
torch.library.define(
  f"{_OP_NAMESPACE}::_mla_append_varlen_hip",
  "(Tensor(a!) kv_cache, Tensor kv_new, Tensor cu_seqlens_q, Tensor cache_seqlens, Tensor block_table) -> Tensor seqused",
)


@torch.library.impl(f"{_OP_NAMESPACE}::_mla_append_varlen_hip", "CUDA")  # ROCm tensors dispatch on the CUDA key
def _mla_append_varlen_hip_torch_op(kv_cache, kv_new, cu_seqlens_q, cache_seqlens, block_table):
  return mla_append_varlen(kv_cache, kv_new, cu_seqlens_q, cache_seqlens, block_table)


def _mla_append_varlen_fake(kv_cache, cu_seqlens_q):
  """``seqused`` of the two ragged latent appends (this one and its FP8 twin)."""
  return kv_cache.new_empty((cu_seqlens_q.size(0) - 1,), dtype=torch.int32)


@torch.library.register_fake(f"{_OP_NAMESPACE}::_mla_append_varlen_hip")
def _mla_append_varlen_hip_fake(kv_cache, kv_new, cu_seqlens_q, cache_seqlens, block_table):
  return _mla_append_varlen_fake(kv_cache, cu_seqlens_q)


# ... and into an FP8 pool (ffpa_attn_varlen_with_kvcache_mla_fp8(kv=)): kv_cache (float8_e4m3fn) is written in place with the quantised rows
torch.library.define(
  f"{_OP_NAMESPACE}::_mla_fp8_append_varlen_hip",
  "(Tensor(a!) kv_cache, Tensor kv_new, float kv_scale, Tensor cu_seqlens_q, Tensor cache_seqlens, Tensor block_table) -> Tensor seqused",
)


@torch.library.impl(f"{_OP_NAMESPACE}::_mla_fp8_append_varlen_hip", "CUDA")  # ROCm tensors dispatch on the CUDA key
def _mla_fp8_append_varlen_hip_torch_op(kv_cache, kv_new, kv_scale, cu_seqlens_q, cache_seqlens, block_table):
  return mla_append_varlen(kv_cache, kv_new, cu_seqlens_q, cache_seqlens, block_table, kv_scale=kv_scale)


@torch.library.register_fake(f"{_OP_NAMESPACE}::_mla_fp8_append_varlen_hip")
def _mla_fp8_append_varlen_hip_fake(kv_cache, kv_new, kv_scale, cu_seqlens_q, cache_seqlens, block_table):
  return _mla_append_varlen_fake(kv_cache, cu_seqlens_q)


# The KV-cache append + rotary (ffpa_attn_with_kvcache(k=, v=, rotary_cos=, rotary_sin=)): the prepare launch in front of the attention launch
def _kvcache_append(name: str, export: str, p, B: int, new_rows: int, q, k_cache, v_cache, k, v, cache_seqlens, block_table, rotary_cos, rotary_sin, rotary_interleaved,
                    causal):
  """What the two appends share — every field ``ffpa_kv_append_params`` and ``ffpa_kv_append_varlen_params`` have in common, the outputs and the call of ``export``.
  ``p``: the export's params with the caller's own fields set (the tensors behind its pointers alive in the caller); ``q`` / ``k`` / ``v``: token rows ``[B, S, H, D]`` or
  packed ``[T, H, D]`` — a row tensor hands over every stride but its last; ``new_rows``: the rows ``k`` / ``v`` hold per sequence (uniform) or in all (ragged)."""
  if not q.is_cuda:
    raise NotImplementedError(f"{name} has no implementation for device '{q.device.type}' (the HIP kernel needs a GPU tensor)")
  lib = load_library()
  rot = rotary_cos is not None
  q_rot = torch.empty(tuple(q.shape) if rot else (0,), dtype=q.dtype, device=q.device)
  seqused = torch.empty((B,), dtype=torch.int32, device=q.device)
  if B <= 0:
    return q_rot, seqused
  for nm, t in (("k_cache", k_cache), ("v_cache", v_cache)):
    if not _layout_ok(t):
      raise ValueError(f"{name}: {nm} is written in place and needs head-dim stride 1, strides that are multiples of 8 elements and a 16-byte aligned base")
  k, v = _rows(k), _rows(v)
  if rot:
    q = _rows(q)
  cache_seqlens = cache_seqlens.contiguous()
  n = q.dim() - 1
  p.k_cache, p.v_cache = k_cache.data_ptr(), v_cache.data_ptr()
  p.seqused, p.cache_seqlens = seqused.data_ptr(), cache_seqlens.data_ptr()
  p.batch, p.heads_q, p.heads_kv, p.head_dim = B, q.size(-2), k_cache.size(2), q.size(-1)
  p.k_cache_stride[:] = list(k_cache.stride()[:3])
  p.v_cache_stride[:] = list(v_cache.stride()[:3])
  if new_rows > 0:
    p.k, p.v = k.data_ptr(), v.data_ptr()
    p.k_stride[:] = list(k.stride()[:n])
    p.v_stride[:] = list(v.stride()[:n])
  if rot:
    p.q, p.q_rot = q.data_ptr(), q_rot.data_ptr()
    p.q_stride[:] = list(q.stride()[:n])
    p.q_rot_stride[:] = list(q_rot.stride()[:n])
    p.rotary_cos, p.rotary_sin = rotary_cos.data_ptr(), rotary_sin.data_ptr()
    p.seqlen_ro = rotary_cos.size(0)
    p.rotary_dim = 2 * rotary_cos.size(1)
    p.rotary_interleaved = 1 if rotary_interleaved else 0
  p.causal = 1 if causal else 0
  p.dtype = _DTYPE[q.dtype]
  kv = None
  if block_table is not None:
    kv, block_table = _paged_kv_of(block_table, k_cache, v_cache)
  else:
    p.capacity = k_cache.size(1)
  rc = _call_on_stream(getattr(lib, export), q.device, ctypes.byref(p), ctypes.byref(kv) if kv is not None else None)
  if rc != 0:
    _raise_status(lib, rc, export)
  return q_rot, seqused


def kvcache_append(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, k: "torch.Tensor | None", v: "torch.Tensor | None", cache_seqlens: torch.Tensor,
                   block_table: "torch.Tensor | None" = None, rotary_cos: "torch.Tensor | None" = None, rotary_sin: "torch.Tensor | None" = None,
                   rotary_interleaved: bool = True, causal: bool = False):
  """One launch of ``ffpa_attn_kvcache_append``: ``k`` / ``v [B, Snew, Hkv, D]`` written into the caches in place at ``cache_seqlens[b] + i`` (``k`` rotated when
  ``rotary_cos`` / ``rotary_sin [seqlen_ro, rotary_dim / 2]`` are given), -> ``(q_rot, seqused)``: ``q [B, Sq, Hq, D]`` rotated (an empty tensor without rotary) and
  the int32 ``[B]`` post-append lengths ``min(max(cache_seqlens, 0) + Snew, capacity)``.  Contiguous caches ``[B, capacity, Hkv, D]``, or page pools
  ``[num_pages, page_size, Hkv, D]`` with ``block_table``.  Asynchronous, nothing read back to the host."""
  B, Sq = q.shape[:2]
  if k is None:
    k = v = q.new_empty((B, 0, k_cache.size(2), q.size(-1)))
  p = _stamped(FfpaKvAppendParams)
  p.seqlen_q, p.seqlen_new = Sq, k.size(1)
  return _kvcache_append("ffpa_attn::_kvcache_append_hip", "ffpa_attn_kvcache_append", p, B, k.size(1), q, k_cache, v_cache, k, v, cache_seqlens, block_table, rotary_cos,
                         rotary_sin, rotary_interleaved, causal)


# k_cache / v_cache are written in place: the schema says so (Tensor(a!) / Tensor(b!)), so that functionalization and torch.compile see the writes
torch.library.define(
  f"{_OP_NAMESPACE}::_kvcache_append_hip",
  "(Tensor q, Tensor(a!) k_cache, Tensor(b!) v_cache, Tensor? k, Tensor? v, Tensor cache_seqlens, Tensor? block_table, Tensor? rotary_cos, "
  "Tensor? rotary_sin, bool rotary_interleaved, bool causal) -> (Tensor q_rot, Tensor seqused)",
)


@torch.library.impl(f"{_OP_NAMESPACE}::_kvcache_append_hip", "CUDA")  # ROCm tensors dispatch on the CUDA key
def _kvcache_append_hip_torch_op(q, k_cache, v_cache, k, v, cache_seqlens, block_table, rotary_cos, rotary_sin, rotary_interleaved, causal):
  return kvcache_append(q, k_cache, v_cache, k, v, cache_seqlens, block_table, rotary_cos, rotary_sin, rotary_interleaved, causal)


@torch.library.register_fake(f"{_OP_NAMESPACE}::_kvcache_append_hip")
def _kvcache_append_hip_fake(q, k_cache, v_cache, k, v, cache_seqlens, block_table, rotary_cos, rotary_sin, rotary_interleaved, causal):
  q_rot = q.new_empty(tuple(q.shape) if rotary_cos is not None else (0,))
  return q_rot, q.new_empty((q.size(0),), dtype=torch.int32)


# The same for a ragged step (ffpa_attn_varlen_with_kvcache): token rows packed by cu_seqlens_q, optional per-token rotary positions
def kvcache_append_varlen(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, k: torch.Tensor, v: torch.Tensor, cu_seqlens_q: torch.Tensor,
                          cache_seqlens: torch.Tensor, block_table: "torch.Tensor | None" = None, rotary_cos: "torch.Tensor | None" = None,
                          rotary_sin: "torch.Tensor | None" = None, positions: "torch.Tensor | None" = None, rotary_interleaved: bool = True, causal: bool = False):
  """One launch of ``ffpa_attn_kvcache_append_varlen``: ``k`` / ``v [T, Hkv, D]``, packed by the int32 device ``cu_seqlens_q [B + 1]`` like ``q [T, Hq, D]``, written
  into the caches in place — key i of sequence b at ``cache_seqlens[b] + i`` (``k`` rotated when ``rotary_cos`` / ``rotary_sin`` are given: at that position, or at
  ``positions[t]`` with the int32 ``positions [T]``) -> ``(q_rot, seqused)``: ``q`` rotated (an empty tensor without rotary) and the int32 ``[B]`` post-append lengths
  ``min(max(cache_seqlens, 0) + Sq_b, capacity)``.  Contiguous caches ``[B, capacity, Hkv, D]``, or page pools with ``block_table``.  Token rows at or past
  ``cu_seqlens_q[B]`` write nothing.  Asynchronous, nothing read back to the host."""
  cu_seqlens_q = cu_seqlens_q.contiguous()
  p = _stamped(FfpaKvAppendVarlenParams)
  p.cu_seqlens_q, p.total_q = cu_seqlens_q.data_ptr(), q.size(0)
  if rotary_cos is not None and positions is not None:
    positions = positions.contiguous()
    p.positions = positions.data_ptr()
  return _kvcache_append("ffpa_attn::_kvcache_append_varlen_hip", "ffpa_attn_kvcache_append_varlen", p, cu_seqlens_q.numel() - 1, q.size(0), q, k_cache, v_cache, k, v,
                         cache_seqlens, block_table, rotary_cos, rotary_sin, rotary_interleaved, causal)


torch.library.define(
  f"{_OP_NAMESPACE}::_kvcache_append_varlen_hip",
  "(Tensor q, Tensor(a!) k_cache, Tensor(b!) v_cache, Tensor k, Tensor v, Tensor cu_seqlens_q, Tensor cache_seqlens, Tensor? block_table, Tensor? rotary_cos, "
  "Tensor? rotary_sin, Tensor? positions, bool rotary_interleaved, bool causal) -> (Tensor q_rot, Tensor seqused)",
)


@torch.library.impl(f"{_OP_NAMESPACE}::_kvcache_append_varlen_hip", "CUDA")  # ROCm tensors dispatch on the CUDA key
def _kvcache_append_varlen_hip_torch_op(q, k_cache, v_cache, k, v, cu_seqlens_q, cache_seqlens, block_table, rotary_cos, rotary_sin, positions, rotary_interleaved,
                                        causal):
  return kvcache_append_varlen(q, k_cache, v_cache, k, v, cu_seqlens_q, cache_seqlens, block_table, rotary_cos, rotary_sin, positions, rotary_interleaved, causal)


@torch.library.register_fake(f"{_OP_NAMESPACE}::_kvcache_append_varlen_hip")
def _kvcache_append_varlen_hip_fake(q, k_cache, v_cache, k, v, cu_seqlens_q, cache_seqlens, block_table, rotary_cos, rotary_sin, positions, rotary_interleaved,
                                    causal):
  q_rot = q.new_empty(tuple(q.shape) if rotary_cos is not None else (0,))
  return q_rot, q.new_empty((cu_seqlens_q.size(0) - 1,), dtype=torch.int32)


# The merge of two attention states (ffpa_merge_attn_states; the last launch of ffpa_attn_with_kvcache_cascade)
def check_merge_states(o_a: torch.Tensor, lse_a: torch.Tensor, o_b: torch.Tensor, lse_b: torch.Tensor, name: str = "ffpa_merge_attn_states") -> None:
  """Host-side checks of a merge (types, shapes, dtypes, devices: nothing read from the device).  ``o_x [T, H, D]`` fp16 / bf16, ``lse_x [H, T]`` fp32."""
  for nm, t in (("o_a", o_a), ("lse_a", lse_a), ("o_b", o_b), ("lse_b", lse_b)):
    if not isinstance(t, torch.Tensor):
      raise TypeError(f"{name}: {nm} must be a tensor, got {type(t).__name__}")
  if o_a.dtype not in _DTYPE or o_b.dtype != o_a.dtype:
    raise TypeError(f"{name} only supports fp16/bf16 o_a / o_b of one dtype, got {o_a.dtype}, {o_b.dtype}")
  if lse_a.dtype != torch.float32 or lse_b.dtype != torch.float32:
    raise TypeError(f"{name}: lse_a / lse_b must be float32, got {lse_a.dtype}, {lse_b.dtype}")
  if o_a.dim() != 3 or o_a.shape != o_b.shape:
    raise ValueError(f"{name}: o_a {tuple(o_a.shape)} and o_b {tuple(o_b.shape)} must be [tokens, heads, head_dim] of one shape")
  T, H, D = o_a.shape
  if D % 8 != 0 or D <= 0 or D > 1024:
    raise ValueError(f"{name}: head dim {D} is not a multiple of 8 in [8, 1024]")
  for nm, t in (("lse_a", lse_a), ("lse_b", lse_b)):
    if tuple(t.shape) != (H, T):
      raise ValueError(f"{name}: {nm} must be [heads={H}, tokens={T}], got {tuple(t.shape)}")
  dev = o_a.device
  for nm, t in (("o_b", o_b), ("lse_a", lse_a), ("lse_b", lse_b)):
    if t.device != dev:
      raise ValueError(f"{name}: {nm} must be on o_a's device, got {t.device} and {dev}")


def merge_states(o_a: torch.Tensor, lse_a: torch.Tensor, o_b: torch.Tensor, lse_b: torch.Tensor, return_lse: bool = True):
  """One launch of ``ffpa_attn_merge_states``: ``(o [T, H, D], lse [H, T] fp32 | None)`` — the attention over the union of the two key sets whose attentions are
  ``(o_a, lse_a)`` and ``(o_b, lse_b)``.  Asynchronous, nothing read back to the host."""
  name = "ffpa_attn::_merge_states_hip"
  check_merge_states(o_a, lse_a, o_b, lse_b, name)
  if not o_a.is_cuda:
    raise NotImplementedError(f"{name} has no implementation for device '{o_a.device.type}' (the HIP kernel needs a GPU tensor)")
  lib = load_library()
  T, H, D = o_a.shape
  o = torch.empty((T, H, D), dtype=o_a.dtype, device=o_a.device)
  lse = torch.empty((H, T), dtype=torch.float32, device=o_a.device) if return_lse else None
  if T == 0 or H == 0:
    return o, lse
  o_a, o_b = _rows(o_a), _rows(o_b)
  lse_a = lse_a if lse_a.stride(1) == 1 and lse_a.stride(0) >= 0 else lse_a.contiguous()
  lse_b = lse_b if lse_b.stride(1) == 1 and lse_b.stride(0) >= 0 else lse_b.contiguous()
  p = _stamped(FfpaMergeStatesParams)
  p.o_a, p.o_b, p.o = o_a.data_ptr(), o_b.data_ptr(), o.data_ptr()
  p.lse_a, p.lse_b = lse_a.data_ptr(), lse_b.data_ptr()
  p.lse = lse.data_ptr() if lse is not None else None
  p.tokens, p.heads, p.head_dim = T, H, D
  p.dtype = _DTYPE[o.dtype]
  p.o_a_stride[:] = list(o_a.stride()[:2])
  p.o_b_stride[:] = list(o_b.stride()[:2])
  p.o_stride[:] = list(o.stride()[:2])
  p.lse_a_stride_head, p.lse_b_stride_head = lse_a.stride(0), lse_b.stride(0)
  p.lse_stride_head = lse.stride(0) if lse is not None else 0
  rc = _call_on_stream(lib.ffpa_attn_merge_states, o.device, ctypes.byref(p))
  if rc != 0:
    _raise_status(lib, rc, "ffpa_attn_merge_states")
  return o, lse


torch.library.define(f"{_OP_NAMESPACE}::_merge_states_hip", "(Tensor o_a, Tensor lse_a, Tensor o_b, Tensor lse_b) -> (Tensor o, Tensor lse)")


@torch.library.impl(f"{_OP_NAMESPACE}::_merge_states_hip", "CUDA")  # ROCm tensors dispatch on the CUDA key
def _merge_states_hip_torch_op(o_a, lse_a, o_b, lse_b):
  return merge_states(o_a, lse_a, o_b, lse_b)


@torch.library.register_fake(f"{_OP_NAMESPACE}::_merge_states_hip")
def _merge_states_hip_fake(o_a, lse_a, o_b, lse_b):
  check_merge_states(o_a, lse_a, o_b, lse_b, "ffpa_attn::_merge_states_hip")
  T, H, D = o_a.shape
  return o_a.new_empty((T, H, D)), o_a.new_empty((H, T), dtype=torch.float32)


# The plan launch of a shared-prefix step over the MLA latent cache (ffpa_attn_with_kvcache_mla_cascade: between the append and the two attention launches)
def check_mla_cascade_plan(lens: torch.Tensor, block_table: torch.Tensor, cu_group_seqs: "torch.Tensor | None", shared_prefix_len: "torch.Tensor | None",
                           shared_prefix_len_host: int, page_size: int, seqlen_q: int, capacity: int, name: str = "ffpa_attn::_mla_cascade_plan_hip") -> "tuple[int, int, int]":
  """Host-side checks of a plan launch (types, shapes, dtypes, devices: nothing read from the device) -> ``(B, G, W)``."""
  for nm, t in (("lens", lens), ("block_table", block_table)):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.int32:
      raise TypeError(f"{name}: {nm} must be an int32 tensor")
  if lens.dim() != 1 or lens.numel() < 1:
    raise ValueError(f"{name}: lens must be a 1-D int32 tensor [batch >= 1], got {tuple(lens.shape)}")
  B = lens.numel()
  if block_table.dim() != 2 or block_table.size(0) != B or block_table.size(1) == 0 or block_table.device != lens.device:
    raise ValueError(f"{name}: block_table must be a 2-D int32 tensor [batch={B}, pages_per_seq >= 1] on the device of lens")
  G = 1
  if cu_group_seqs is not None:
    if cu_group_seqs.dtype != torch.int32:
      raise TypeError(f"{name}: cu_group_seqs must be int32, got {cu_group_seqs.dtype}")
    if cu_group_seqs.dim() != 1 or cu_group_seqs.numel() < 2 or cu_group_seqs.device != lens.device:
      raise ValueError(f"{name}: cu_group_seqs must be a 1-D int32 tensor [groups + 1] on the device of lens, got {tuple(cu_group_seqs.shape)} on {cu_group_seqs.device}")
    G = cu_group_seqs.numel() - 1
  if shared_prefix_len is not None:
    if shared_prefix_len.dtype != torch.int32:
      raise TypeError(f"{name}: a tensor shared_prefix_len must be int32, got {shared_prefix_len.dtype}")
    if tuple(shared_prefix_len.shape) != (G,) or shared_prefix_len.device != lens.device:
      raise ValueError(f"{name}: a tensor shared_prefix_len must be [groups={G}] on the device of lens, got {tuple(shared_prefix_len.shape)} on {shared_prefix_len.device}")
  elif shared_prefix_len_host < 0:
    raise ValueError(f"{name}: shared_prefix_len must be non-negative, got {shared_prefix_len_host}")
  W = block_table.size(1)
  if page_size <= 0 or page_size % 64 != 0:
    raise ValueError(f"{name}: page_size ({page_size}) must be a positive multiple of 64")
  if seqlen_q < 1 or not 0 < capacity <= W * page_size:
    raise ValueError(f"{name}: seqlen_q ({seqlen_q}) must be at least 1 and capacity ({capacity}) in (0, pages_per_seq * page_size = {W * page_size}]")
  return B, G, W


def _mla_cascade_plan_outputs(lens: torch.Tensor, B: int, G: int, W: int):
  new = lambda *shape: lens.new_empty(shape, dtype=torch.int32)
  return new(G + 1), new(G), new(G, W), new(B, W), new(B)


def mla_cascade_plan(lens: torch.Tensor, block_table: torch.Tensor, cu_group_seqs: "torch.Tensor | None", shared_prefix_len: "torch.Tensor | None",
                     shared_prefix_len_host: int, page_size: int, seqlen_q: int, causal: bool, capacity: int):
  """One launch of ``ffpa_attn_mla_cascade_plan`` -> ``(cu_q_prefix [G + 1], prefix_lens [G], prefix_table [G, W], suffix_table [B, W], suffix_lens [B])``, all
  int32 on the device of ``lens`` (the keys every sequence holds after the step's append, not clamped): the effective prefix of every group of
  ``cu_group_seqs`` (None: one group) — the stated one (``shared_prefix_len [G]`` on the device, or the host int) cut back to what every sequence of the group
  holds (and, under ``causal``, to what its first query token may see) and rounded down to whole pages —, the packed queries' boundaries by group, the block-table
  row of every group's first sequence, every sequence's row shifted left by its group's prefix pages, and the suffix lengths.  Asynchronous, nothing read back to
  the host."""
  name = "ffpa_attn::_mla_cascade_plan_hip"
  B, G, W = check_mla_cascade_plan(lens, block_table, cu_group_seqs, shared_prefix_len, shared_prefix_len_host, page_size, seqlen_q, capacity, name)
  if not lens.is_cuda:
    raise NotImplementedError(f"{name} has no implementation for device '{lens.device.type}' (the HIP kernel needs a GPU tensor)")
  lib = load_library()
  lens = lens.contiguous()
  if block_table.stride(1) != 1 or block_table.data_ptr() % 4 != 0:
    block_table = block_table.contiguous()
  cu_group_seqs = cu_group_seqs.contiguous() if cu_group_seqs is not None else None
  shared_prefix_len = shared_prefix_len.contiguous() if shared_prefix_len is not None else None
  outs = _mla_cascade_plan_outputs(lens, B, G, W)
  p = _stamped(FfpaMlaCascadePlanParams)
  p.cu_group_seqs = cu_group_seqs.data_ptr() if cu_group_seqs is not None else None
  p.shared_prefix_len = shared_prefix_len.data_ptr() if shared_prefix_len is not None else None
  p.lens, p.block_table = lens.data_ptr(), block_table.data_ptr()
  p.cu_q_prefix, p.prefix_lens, p.prefix_table, p.suffix_table, p.suffix_lens = (t.data_ptr() for t in outs)
  p.bt_stride = block_table.stride(0) if B > 1 else W
  p.batch, p.groups, p.pages_per_seq, p.page_size, p.seqlen_q, p.causal, p.capacity = B, G, W, page_size, seqlen_q, 1 if causal else 0, capacity
  p.shared_prefix_len_host = shared_prefix_len_host if shared_prefix_len is None else 0
  rc = _call_on_stream(lib.ffpa_attn_mla_cascade_plan, lens.device, ctypes.byref(p))
  if rc != 0:
    _raise_status(lib, rc, "ffpa_attn_mla_cascade_plan")
  return outs


torch.library.define(
  f"{_OP_NAMESPACE}::_mla_cascade_plan_hip",
  "(Tensor lens, Tensor block_table, Tensor? cu_group_seqs, Tensor? shared_prefix_len, int shared_prefix_len_host, int page_size, int seqlen_q, int causal, "
  "int capacity) -> (Tensor cu_q_prefix, Tensor prefix_lens, Tensor prefix_table, Tensor suffix_table, Tensor suffix_lens)",
)


@torch.library.impl(f"{_OP_NAMESPACE}::_mla_cascade_plan_hip", "CUDA")  # ROCm tensors dispatch on the CUDA key
def _mla_cascade_plan_hip_torch_op(lens, block_table, cu_group_seqs, shared_prefix_len, shared_prefix_len_host, page_size, seqlen_q, causal, capacity):
  return mla_cascade_plan(lens, block_table, cu_group_seqs, shared_prefix_len, shared_prefix_len_host, page_size, seqlen_q, bool(causal), capacity)


@torch.library.register_fake(f"{_OP_NAMESPACE}::_mla_cascade_plan_hip")
def _mla_cascade_plan_hip_fake(lens, block_table, cu_group_seqs, shared_prefix_len, shared_prefix_len_host, page_size, seqlen_q, causal, capacity):
  B, G, W = check_mla_cascade_plan(lens, block_table, cu_group_seqs, shared_prefix_len, shared_prefix_len_host, page_size, seqlen_q, capacity)
  return _mla_cascade_plan_outputs(lens, B, G, W)
