"""``ffpa_mla_index_scores`` without a GPU: every argument refusal of the public call, the C struct's size and the order of the C statuses, the fake op."""

import ctypes

import pytest
import torch

import ffpa_attn_amd
from ffpa_attn_amd import hip

scores_of = ffpa_attn_amd.ffpa_mla_index_scores
SYMBOL = "ffpa_attn_mla_index_scores"


@pytest.fixture(scope="module")
def lib():
  if not hip.library_available():
    from ffpa_attn_amd import build

    build.build()
  return hip.load_library()


def _good(T=4, Hi=64, B=2, W=3, pages=8, page=64, dtype=torch.bfloat16):
  return dict(q_index=torch.zeros(T, Hi, 128, dtype=dtype), k_index_cache=torch.zeros(pages, page, 128, dtype=dtype), weights=torch.zeros(T, Hi),
              cache_seqlens=torch.full((B,), 100, dtype=torch.int32), block_table=torch.zeros(B, W, dtype=torch.int32), max_seqlen_k=128)


def _grad(t):
  return t.clone().requires_grad_()


@pytest.mark.parametrize("over, exc, text", [
  (dict(q_index=[1.0]), TypeError, "q_index must be a tensor"),
  (dict(weights=lambda a: _grad(a["weights"])), NotImplementedError, "inference only: weights requires grad"),
  (dict(q_index=lambda a: a["q_index"].float()), TypeError, "q_index must be bf16 or fp16"),
  (dict(k_index_cache=lambda a: a["k_index_cache"].half()), TypeError, "k_index_cache must have q_index's dtype"),
  (dict(k_index_cache=lambda a: a["k_index_cache"].to(torch.float8_e4m3fn)), TypeError, "FP8 index keys are not served"),
  (dict(weights=lambda a: a["weights"].bfloat16()), TypeError, "weights must be torch.float32"),
  (dict(cache_seqlens=lambda a: a["cache_seqlens"].long()), TypeError, "cache_seqlens must be an int32 tensor"),
  (dict(block_table=lambda a: a["block_table"].long()), TypeError, "block_table must be an int32 tensor"),
  (dict(max_seqlen_k=128.0), TypeError, "max_seqlen_k must be an int"),
  (dict(max_seqlen_k=0), ValueError, r"max_seqlen_k must lie in \[1, 2\^30\]"),
  (dict(q_index=lambda a: torch.zeros(4, 64, 64, dtype=torch.bfloat16)), ValueError, r"q_index must be \[T, Hi, 128\]"),
  (dict(q_index=lambda a: torch.zeros(4, 16, 128, dtype=torch.bfloat16), weights=torch.zeros(4, 16)), NotImplementedError, r"built for Hi in \(32, 64\)"),
  (dict(k_index_cache=lambda a: torch.zeros(8, 64, 2, 128, dtype=torch.bfloat16)), ValueError, "ONE head"),
  (dict(k_index_cache=lambda a: torch.zeros(8, 64, 64, dtype=torch.bfloat16)), ValueError, "k_index_cache must be"),
  (dict(k_index_cache=lambda a: torch.zeros(8, 48, 128, dtype=torch.bfloat16)), ValueError, "page size must be a positive multiple of 64"),
  (dict(block_table=None), ValueError, r"without a block_table k_index_cache must be \[B=2, capacity, 128\]"),
  (dict(block_table=None, k_index_cache=lambda a: torch.zeros(2, 100, 128, dtype=torch.bfloat16)), ValueError, "capacity must be a positive multiple of 64"),
  (dict(weights=torch.zeros(4, 32)), ValueError, "weights must be"),
  (dict(cu_seqlens_q=torch.zeros(2, dtype=torch.int32)), ValueError, "cu_seqlens_q must be an int32 tensor"),
  (dict(cache_seqlens=torch.zeros(3, dtype=torch.int32), block_table=torch.zeros(3, 3, dtype=torch.int32)), ValueError, "T must be a multiple of B=3"),
  (dict(block_table=torch.zeros(3, 3, dtype=torch.int32)), ValueError, "one row per SEQUENCE"),
  (dict(q_index=lambda a: torch.zeros(4, 64, 256, dtype=torch.bfloat16)[:, :, ::2]), ValueError, "q_index must have a contiguous last dimension"),
  (dict(q_index=lambda a: torch.zeros(4, 64, 132, dtype=torch.bfloat16)[:, :, :128]), ValueError, "strides of q_index must be multiples of 8"),
  (dict(k_index_cache=lambda a: torch.zeros(8, 64, 132, dtype=torch.bfloat16)[:, :, :128]), ValueError, "strides of k_index_cache must be multiples of 8"),
  (dict(weights=lambda a: a["weights"].to("meta")), ValueError, "weights must be on q_index's device"),
])
def test_argument_errors(over, exc, text):
  a = _good()
  a.update({k_: v(a) if callable(v) else v for k_, v in over.items()})
  with pytest.raises(exc, match=text):
    scores_of(a.pop("q_index"), a.pop("k_index_cache"), a.pop("weights"), a.pop("cache_seqlens"), a.pop("block_table"), **a)


def test_exported_and_no_tokens_launch_nothing():
  assert "ffpa_mla_index_scores" in ffpa_attn_amd.__all__ and scores_of is ffpa_attn_amd.kvcache.ffpa_mla_index_scores
  assert hip.MLA_INDEX_CHUNK_KEYS in (256, 512, 1024)
  a = _good(T=0)
  out = scores_of(a["q_index"], a["k_index_cache"], a["weights"], a["cache_seqlens"], a["block_table"], max_seqlen_k=77)
  assert out.shape == (0, 77) and out.dtype == torch.float32


def test_the_op_has_a_fake():
  a = {k_: (v.to("meta") if isinstance(v, torch.Tensor) else v) for k_, v in _good(T=6, Hi=32).items()}
  out = torch.ops.ffpa_attn._mla_index_scores_hip(a["q_index"], a["k_index_cache"], a["weights"], a["cache_seqlens"], a["block_table"], 1000, None, True)
  assert out.shape == (6, 1000) and out.dtype == torch.float32 and out.device.type == "meta"
  out = scores_of(a["q_index"], a["k_index_cache"], a["weights"], a["cache_seqlens"], a["block_table"], max_seqlen_k=40, causal=False)
  assert out.shape == (6, 40) and out.dtype == torch.float32


def test_the_three_launches_compile_as_one_graph_on_meta_tensors():
  a = {k_: (v.to("meta") if isinstance(v, torch.Tensor) else v) for k_, v in _good(T=6, Hi=64, pages=40).items()}
  ql, latent = torch.empty(6, 16, 576, dtype=torch.bfloat16, device="meta"), torch.empty(40, 64, 1, 576, dtype=torch.bfloat16, device="meta")

  def f(q, k, w, lens, table, ql, latent):
    s = scores_of(q, k, w, lens, table, max_seqlen_k=2560)
    idx, n = ffpa_attn_amd.ffpa_mla_sparse_topk_slots(s, 320, lens, table, 64)
    return ffpa_attn_amd.ffpa_attn_with_kvcache_mla_sparse(ql, latent, 512, idx, topk_lens=n, softmax_scale=0.07) * 2, s

  args = (a["q_index"], a["k_index_cache"], a["weights"], a["cache_seqlens"], a["block_table"], ql, latent)
  for fn in (f, torch.compile(f, fullgraph=True, backend="eager")):
    out, s = fn(*args)
    assert out.shape == (6, 16, 512) and out.device.type == "meta" and s.shape == (6, 2560) and s.dtype == torch.float32


# ----------------------------------------------------------------------------- the C statuses, in their order
_KEEP = []
_POINTERS = ("q_index", "k_index_cache", "weights", "cache_seqlens", "cu_seqlens_q", "block_table", "scores")


def _params(over):
  buf = (ctypes.c_char * 4096)()
  _KEEP.append(buf)
  base = (ctypes.addressof(buf) + 15) & ~15
  p = hip._stamped(hip.FfpaMlaIndexScoresParams)
  for f in _POINTERS:
    setattr(p, f, base)
  p.q_stride[0], p.q_stride[1], p.k_stride[0], p.k_stride[1] = 64 * 128, 128, 64 * 128, 128
  p.weights_stride, p.block_table_stride, p.scores_stride = 64, 8, 4096
  p.T, p.heads, p.head_dim, p.N, p.B, p.W, p.page_size, p.num_pages, p.causal, p.dtype = 8, 64, 128, 4096, 2, 8, 64, 16, 1, 0
  for k_, v_ in over.items():
    if k_ in ("q_stride", "k_stride"):
      getattr(p, k_)[v_[0]] = v_[1]
    else:
      setattr(p, k_, (base + v_) if isinstance(v_, int) and k_ in _POINTERS else v_)
  return p


@pytest.mark.parametrize("over, status, text", [
  # ... each in front of the next: a pair of faults answers with the earlier one
  (dict(struct_size=160, reserved=1), 10, b"ffpa_mla_index_scores_params ABI mismatch: size 160 (want 168)"),
  (dict(reserved2=1, dtype=2), 10, b"reserved2"),
  (dict(dtype=2, head_dim=64), 2, b"dtype 2"),
  (dict(head_dim=64, heads=16), 3, b"head_dim=64"),
  (dict(heads=16, T=-1), 7, b"heads=16"),
  (dict(T=-1, B=0), 4, b"T=-1"),
  (dict(N=(1 << 30) + 1), 4, b"[1, 2^30]"),
  (dict(B=3, cu_seqlens_q=None), 4, b"divide T=8"),
  (dict(causal=2, page_size=32), 4, b"causal=2"),
  (dict(page_size=96, W=0), 4, b"page_size=96"),
  (dict(block_table=None, page_size=0), 4, b"page_size=0"),
  (dict(W=0, chunk_keys=100), 4, b"W=0"),
  (dict(num_pages=0), 4, b"num_pages=0"),
  (dict(chunk_keys=100, scores_stride=-1), 4, b"chunk_keys=100"),
  (dict(T=1 << 15, N=1 << 20, scores_stride=-1), 4, b"grid of 33554432 workgroups is too large (at most 2^24)"),
  (dict(weights_stride=-1, q_stride=(1, 4)), 5, b"stride -1"),
  (dict(q_stride=(1, 4), scores_stride=8), 5, b"multiples of 8"),
  (dict(k_stride=(1, 64)), 5, b"at least 128 elements apart"),
  (dict(scores_stride=4095, scores=None), 5, b"scores_stride=4095 is smaller than N=4096"),
  (dict(scores=None, q_index=2), 1, b"must be non-NULL"),
  (dict(k_index_cache=8, weights=2), 6, b"16-byte aligned"),
  (dict(cu_seqlens_q=2), 6, b"4-byte aligned"),
])
def test_the_statuses_and_their_order(lib, over, status, text):
  assert ctypes.sizeof(hip.FfpaMlaIndexScoresParams) == 168 and SYMBOL in hip.EXPORTS and hip.ABI_VERSION == 7
  p = _params(over)
  assert lib.ffpa_attn_mla_index_scores(ctypes.byref(p), None) == status, lib.ffpa_attn_last_error()
  assert text in lib.ffpa_attn_last_error(), lib.ffpa_attn_last_error()
  assert lib.ffpa_attn_mla_index_scores(None, None) == 1
  assert lib.ffpa_attn_mla_index_scores(ctypes.byref(_params(dict(T=0, scores=None, block_table=None, W=0, num_pages=0))), None) == 0
