"""The FP8 index-key calls without a GPU: the row and page format at byte level, the public names and exports, the C structs' sizes against the header, the
refusals of the public calls and of the C layer (in their order), the fake ops."""

import ctypes
import os
import subprocess

import pytest
import torch

import ffpa_attn_amd
from ffpa_attn_amd import hip, pack_index_key_pages, quantize_index_rows, unpack_index_key_pages

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E4M3 = torch.float8_e4m3fn


@pytest.fixture(scope="module")
def lib():
  if not hip.library_available():
    from ffpa_attn_amd import build

    build.build()
  return hip.load_library()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_quantize_index_rows_on_its_edges(dtype):
  x = torch.randn(6, 128).to(dtype)
  x[0] = 0                                   # the 1e-4 floor: 1e-4 / 448 = 2.23e-7 rounds up to 2^-22
  x[1], x[1, 3] = 1.0, -448.0                # amax = 448: s = 1 exactly, a power of two stays
  x[2], x[2, 9] = 1.0, 452.0                 # just above (the next bf16): the next power of two
  x[3], x[3, 0] = 0.25, 448.0 * 2.0 ** -7    # a boundary below one
  codes, scale = quantize_index_rows(x)
  assert codes.dtype == E4M3 and codes.shape == x.shape and scale.dtype == torch.float32 and scale.shape == (6,)
  assert scale[:4].tolist() == [2.0 ** -22, 1.0, 2.0, 2.0 ** -7]
  assert not codes[0].float().any() and codes[1, 3].float() == -448 and codes[2, 9].float() == 224 and codes[3, 0].float() == 448
  s = x.float().abs().amax(-1).clamp(min=1e-4) / 448
  assert bool((scale >= s).all() and (scale < 2 * s).all() and ((scale.view(torch.int32) & 0x7FFFFF) == 0).all())
  assert bool(((codes.float() * scale[:, None] - x.float()).abs() <= 16 * scale[:, None]).all())  # (half of e4m3's largest step, 32)
  with pytest.raises(ValueError, match=r"\[\.\.\., 128\]"):
    quantize_index_rows(torch.zeros(4, 64))


def test_pack_is_two_planes_per_page_and_unpack_inverts_it():
  codes, scale = quantize_index_rows(torch.randn(3, 64, 128))
  pages = pack_index_key_pages(codes, scale)
  assert pages.dtype == torch.uint8 and pages.shape == (3, 64, 132) and pages.is_contiguous()
  flat = pages.view(3, 64 * 132)
  assert torch.equal(flat[:, :64 * 128], codes.view(torch.uint8).view(3, -1))          # first the codes, row-major
  assert torch.equal(flat[:, 64 * 128:], scale.view(torch.uint8).view(3, -1))          # then the float32 scales
  assert torch.equal(flat[1, 64 * 128 + 4 * 5:64 * 128 + 4 * 6], scale[1, 5:6].view(torch.uint8))
  back = unpack_index_key_pages(pages)
  assert torch.equal(back[0].view(torch.uint8), codes.view(torch.uint8)) and torch.equal(back[1], scale)
  with pytest.raises(ValueError, match="132"):
    unpack_index_key_pages(torch.zeros(3, 64, 128, dtype=torch.uint8))


def test_exports_and_struct_sizes_against_the_header(tmp_path):
  for name in ("ffpa_mla_index_scores_fp8", "ffpa_mla_index_k_append_fp8", "quantize_index_rows", "pack_index_key_pages", "unpack_index_key_pages"):
    assert name in ffpa_attn_amd.__all__ and getattr(ffpa_attn_amd, name) is getattr(ffpa_attn_amd.kvcache, name)
  assert {"ffpa_attn_mla_index_scores_fp8", "ffpa_attn_mla_index_k_append_fp8"} <= set(hip.EXPORTS) and hip.ABI_VERSION == 7
  src, exe = tmp_path / "sizes.c", tmp_path / "sizes"
  src.write_text('#include <stdio.h>\n#include "ffpa_attn.h"\nint main(void) {printf("%zu %zu %d\\n", sizeof(ffpa_mla_index_scores_fp8_params), '
                 'sizeof(ffpa_mla_index_k_append_fp8_params), FFPA_ATTN_ABI_VERSION);\nreturn 0;}\n')
  subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
  sizes = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
  assert sizes == [ctypes.sizeof(hip.FfpaMlaIndexScoresFp8Params), ctypes.sizeof(hip.FfpaMlaIndexKAppendFp8Params), 7] == [152, 112, 7]


def _good(T=4, Hi=64, B=2, W=3, pages=8, page=64):
  return dict(q_index=torch.zeros(T, Hi, 128).to(E4M3), k_index_cache=torch.zeros(pages, page, 132, dtype=torch.uint8), weights=torch.zeros(T, Hi),
              cache_seqlens=torch.full((B,), 100, dtype=torch.int32), block_table=torch.zeros(B, W, dtype=torch.int32), max_seqlen_k=128)


@pytest.mark.parametrize("over, exc, text", [
  (dict(weights=[1.0]), TypeError, "weights must be a tensor"),
  (dict(weights=lambda a: a["weights"].clone().requires_grad_()), NotImplementedError, "inference only: weights requires grad"),
  (dict(q_index=lambda a: a["q_index"].bfloat16()), TypeError, "q_index must be torch.float8_e4m3fn"),
  (dict(k_index_cache=lambda a: a["k_index_cache"].view(E4M3)), TypeError, "k_index_cache must be torch.uint8"),
  (dict(q_index=lambda a: torch.zeros(4, 16, 128).to(E4M3), weights=torch.zeros(4, 16)), NotImplementedError, r"built for Hi in \(32, 64\)"),
  (dict(k_index_cache=lambda a: torch.zeros(8, 64, 128, dtype=torch.uint8)), ValueError, "128 codes and a float32 scale per key"),
  (dict(k_index_cache=lambda a: torch.zeros(8, 48, 132, dtype=torch.uint8)), ValueError, "page size must be a positive multiple of 64"),
  (dict(block_table=None), ValueError, r"without a block_table k_index_cache must be \[B=2, capacity, 132\]"),
  (dict(k_index_cache=lambda a: torch.zeros(8, 64, 136, dtype=torch.uint8)[:, :, :132]), ValueError, r"64 \* 132 contiguous bytes"),
  (dict(q_index=lambda a: torch.zeros(4, 64, 136).to(E4M3)[:, :, :128]), ValueError, "strides of q_index must be multiples of 16"),
  (dict(weights=lambda a: a["weights"].to("meta")), ValueError, "weights must be on q_index's device"),
])
def test_argument_errors_of_the_score_call(over, exc, text):
  a = _good()
  a.update({k_: v(a) if callable(v) else v for k_, v in over.items()})
  with pytest.raises(exc, match=text):
    ffpa_attn_amd.ffpa_mla_index_scores_fp8(a.pop("q_index"), a.pop("k_index_cache"), a.pop("weights"), a.pop("cache_seqlens"), a.pop("block_table"), **a)


@pytest.mark.parametrize("over, exc, text", [
  (dict(k_index=lambda a: a["k_index"].float()), TypeError, "k_index must be bf16 or fp16"),
  (dict(k_index=torch.zeros(4, 2, 128, dtype=torch.bfloat16)), ValueError, r"k_index must be \[T, 128\] or \[T, 1, 128\]"),
  (dict(k_index=torch.zeros(5, 128, dtype=torch.bfloat16)), ValueError, "T must be a multiple of B=2"),
  (dict(k_index=torch.zeros(4, 132, dtype=torch.bfloat16)[:, :128]), ValueError, "row stride of k_index must be a multiple of 8"),
])
def test_argument_errors_of_the_append(over, exc, text):
  a = dict(k_index_cache=_good()["k_index_cache"], k_index=torch.zeros(4, 128, dtype=torch.bfloat16), cache_seqlens=torch.zeros(2, dtype=torch.int32),
           block_table=torch.zeros(2, 3, dtype=torch.int32))
  a.update({k_: v(a) if callable(v) else v for k_, v in over.items()})
  with pytest.raises(exc, match=text):
    ffpa_attn_amd.ffpa_mla_index_k_append_fp8(a.pop("k_index_cache"), a.pop("k_index"), a.pop("cache_seqlens"), a.pop("block_table"), **a)


def test_the_ops_have_fakes_and_the_16_bit_call_still_refuses_the_pool():
  a = {k_: (v.to("meta") if isinstance(v, torch.Tensor) else v) for k_, v in _good(T=6, Hi=32).items()}
  k_new = torch.empty(6, 1, 128, dtype=torch.float16, device="meta")

  def f(q, k, w, lens, table, k_new):
    after = ffpa_attn_amd.ffpa_mla_index_k_append_fp8(k, k_new, lens, table)
    return ffpa_attn_amd.ffpa_mla_index_scores_fp8(q, k, w, after, table, max_seqlen_k=1000, causal=False), after

  for fn in (f, torch.compile(f, fullgraph=True, backend="eager")):
    s, after = fn(a["q_index"], a["k_index_cache"], a["weights"], a["cache_seqlens"], a["block_table"], k_new)
    assert s.shape == (6, 1000) and s.dtype == torch.float32 and s.device.type == "meta" and after.shape == (2,) and after.dtype == torch.int32
  assert ffpa_attn_amd.ffpa_mla_index_scores_fp8(a["q_index"][:0], a["k_index_cache"], a["weights"][:0], a["cache_seqlens"], a["block_table"], max_seqlen_k=7).shape == (0, 7)
  b = _good()
  with pytest.raises(TypeError, match="FP8 index keys are not served"):
    ffpa_attn_amd.ffpa_mla_index_scores(b["q_index"].bfloat16(), b["k_index_cache"], b["weights"], b["cache_seqlens"], b["block_table"], max_seqlen_k=128)


# ----------------------------------------------------------------------------- the C statuses, in their order
_KEEP = []


def _params(cls, over):
  buf = (ctypes.c_char * 4096)()
  _KEEP.append(buf)
  base = (ctypes.addressof(buf) + 15) & ~15
  p = hip._stamped(cls)
  pointers = [n for n, t in cls._fields_ if t is ctypes.c_void_p]
  for f in pointers:
    setattr(p, f, base)
  p.k_page_stride, p.block_table_stride, p.T, p.head_dim, p.B, p.W, p.page_size, p.num_pages = 64 * 132, 8, 8, 128, 2, 8, 64, 16
  if cls is hip.FfpaMlaIndexScoresFp8Params:
    p.q_stride[0], p.q_stride[1], p.weights_stride, p.scores_stride, p.heads, p.N, p.causal = 64 * 128, 128, 64, 4096, 64, 4096, 1
  else:
    p.k_index_stride = 128
  for k_, v_ in over.items():
    if k_ == "q_stride":
      p.q_stride[v_[0]] = v_[1]
    else:
      setattr(p, k_, (base + v_) if isinstance(v_, int) and k_ in pointers else v_)
  return p


@pytest.mark.parametrize("call, over, status, text", [
  # ... each in front of the next: a pair of faults answers with the earlier one
  ("scores", dict(struct_size=144, head_dim=64), 10, b"ffpa_mla_index_scores_fp8_params ABI mismatch: size 144 (want 152)"),
  ("scores", dict(head_dim=64, heads=16), 3, b"head_dim=64"),
  ("scores", dict(heads=16, T=-1), 7, b"heads=16"),
  ("scores", dict(T=-1, page_size=96), 4, b"T=-1"),
  ("scores", dict(page_size=96, chunk_keys=100), 4, b"page_size=96"),
  ("scores", dict(chunk_keys=100, q_stride=(1, 8)), 4, b"chunk_keys=100"),
  ("scores", dict(q_stride=(1, 8), k_page_stride=64 * 128), 5, b"multiples of 16 bytes"),
  ("scores", dict(k_page_stride=64 * 128, scores_stride=8), 5, b"a page of 64 keys is 8448 bytes"),
  ("scores", dict(scores_stride=4095, scores=None), 5, b"scores_stride=4095 is smaller than N=4096"),
  ("scores", dict(scores=None, q_index=2), 1, b"must be non-NULL"),
  ("scores", dict(k_index_cache=8, weights=2), 6, b"16-byte aligned"),
  ("append", dict(struct_size=104, dtype=2), 10, b"ffpa_mla_index_k_append_fp8_params ABI mismatch: size 104 (want 112)"),
  ("append", dict(reserved2=1, dtype=2), 10, b"reserved2=1"),
  ("append", dict(dtype=2, head_dim=64), 2, b"dtype 2"),
  ("append", dict(head_dim=64, T=-1), 3, b"head_dim=64"),
  ("append", dict(T=-1, B=0), 4, b"T=-1"),
  ("append", dict(B=3, cu_seqlens_q=None, num_pages=0), 4, b"divide T=8"),
  ("append", dict(num_pages=0, k_index_stride=4), 4, b"num_pages=0"),
  ("append", dict(k_index_stride=4, lens_after=None), 5, b"of 8 elements"),
  ("append", dict(k_page_stride=64 * 128, lens_after=None), 5, b"a page of 64 keys is 8448 bytes"),
  ("append", dict(lens_after=None, k_index=2), 1, b"must be non-NULL"),
  ("append", dict(k_index=8, block_table=2), 6, b"16-byte aligned"),
])
def test_the_statuses_and_their_order(lib, call, over, status, text):
  cls, fn = {"scores": (hip.FfpaMlaIndexScoresFp8Params, lib.ffpa_attn_mla_index_scores_fp8), "append": (hip.FfpaMlaIndexKAppendFp8Params, lib.ffpa_attn_mla_index_k_append_fp8)}[call]
  assert fn(ctypes.byref(_params(cls, over)), None) == status, lib.ffpa_attn_last_error()
  assert text in lib.ffpa_attn_last_error(), lib.ffpa_attn_last_error()
  assert fn(None, None) == 1
