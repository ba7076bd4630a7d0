"""``ffpa_mla_sparse_topk_slots`` / ``ffpa_mla_sparse_slots`` without a GPU: the exports and the C ABI of ``ffpa_attn_mla_sparse_topk_slots`` (statuses and their
order — nothing is launched here), every argument error of the two calls, the ops' fakes, and the definition itself (tests/kvcache_mla_sparse_topk_ref.py) against
brute force and against the two torch helpers the calls supersede on the hot path."""

import ctypes
import itertools
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import ffpa_attn_amd
import kvcache_mla_sparse_topk_ref as TR
from ffpa_attn_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ffpa_mla_sparse_topk_slots", "ffpa_mla_sparse_slots")
SYMBOL = "ffpa_attn_mla_sparse_topk_slots"
topk_slots, slots = ffpa_attn_amd.ffpa_mla_sparse_topk_slots, ffpa_attn_amd.ffpa_mla_sparse_slots


@pytest.fixture(scope="module")
def lib():
  if not hip.library_available():
    from ffpa_attn_amd import build

    build.build()
  return hip.load_library()


# ----------------------------------------------------------------------------- exports
def test_both_names_are_exported():
  for name in NAMES:
    assert name in ffpa_attn_amd.__all__
    assert getattr(ffpa_attn_amd, name) is getattr(ffpa_attn_amd.kvcache, name)


def test_abi_version_stays_7_and_the_symbol_is_exported_and_declared(lib, tmp_path):
  assert hip.ABI_VERSION == 7 and lib.ffpa_attn_query(0) == 7
  assert SYMBOL in hip.EXPORTS and getattr(lib, SYMBOL) is not None
  header = open(os.path.join(ROOT, "include", "ffpa_attn.h")).read()
  declared = set(re.findall(r"^\s*(?:int|size_t|const char\*)\s+(ffpa_attn_\w+)\s*\(", header, flags=re.M))
  assert SYMBOL in declared and declared == set(hip.EXPORTS)
  src = tmp_path / "decl.c"
  src.write_text('#include <stdio.h>\n#include "ffpa_attn.h"\nint main(void){\nvoid* fn = (void*)' + SYMBOL +
                 ';\nprintf("%d %zu %p\\n", FFPA_ATTN_ABI_VERSION, sizeof(ffpa_mla_sparse_topk_params), fn);\nreturn 0;}\n')
  subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-Wno-pedantic", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "decl.o")], check=True)
  assert re.findall(r"typedef struct (\w+)", header).count("ffpa_mla_sparse_topk_params") == 1 and ctypes.sizeof(hip.FfpaMlaSparseTopkParams) == 120


# ----------------------------------------------------------------------------- the C statuses, in their order
_KEEP = []


def _params(over=None, positions=False):
  buf = (ctypes.c_char * 4096)()
  _KEEP.append(buf)
  base = (ctypes.addressof(buf) + 15) & ~15
  p = hip._stamped(hip.FfpaMlaSparseTopkParams)
  if positions:
    p.positions = base
  else:
    p.scores = base
  p.cache_seqlens = p.cu_seqlens_q = p.block_table = p.indices = p.topk_lens = base
  p.row_stride, p.block_table_stride, p.indices_stride = 4096, 8, 64
  p.T, p.N_or_topk, p.topk, p.B, p.W, p.page_size, p.causal = 8, 64 if positions else 4096, 64, 2, 8, 64, 1
  for k_, v_ in (over or {}).items():
    setattr(p, k_, (base + v_) if isinstance(v_, int) and k_ in ("scores", "positions", "cache_seqlens", "cu_seqlens_q", "block_table", "indices", "topk_lens") else v_)
  return p


@pytest.mark.parametrize("over, positions, status, text", [
  (dict(struct_size=112), False, 10, b"ffpa_mla_sparse_topk_params ABI mismatch: size 112 (want 120)"),
  (dict(reserved=1), False, 10, b"reserved"),
  (dict(reserved2=1), False, 10, b"reserved2"),
  (dict(positions=0), False, 1, b"exactly one of scores / positions must be non-NULL (both are)"),
  (dict(scores=None), False, 1, b"exactly one of scores / positions must be non-NULL (neither are)"),
  # ... each in front of the next: both pointers AND topk = 0, topk = 0 AND page_size = 0
  (dict(positions=0, topk=0), False, 1, b"exactly one"),
  (dict(T=-1), False, 4, b"T=-1"),
  (dict(N_or_topk=0), False, 4, b"N_or_topk=0"),
  (dict(N_or_topk=(1 << 30) + 1), False, 4, b"[1, 2^30]"),
  (dict(topk=0), False, 4, b"topk=0 must be positive"),
  (dict(topk=0, page_size=0), False, 4, b"topk=0 must be positive"),
  (dict(topk=32), True, 4, b"positions: N_or_topk=64 must equal topk=32"),
  (dict(B=0), False, 4, b"B=0"),
  (dict(B=3, cu_seqlens_q=None), False, 4, b"divide T=8"),
  (dict(causal=2), False, 4, b"causal=2"),
  (dict(page_size=0), False, 4, b"page_size=0"),
  (dict(page_size=0), True, 4, b"page_size=0"),
  (dict(W=0), False, 4, b"W=0"),
  (dict(page_size=0, indices_stride=8), False, 4, b"page_size=0"),
  (dict(row_stride=-1), False, 5, b"row_stride=-1"),
  (dict(indices_stride=63), False, 5, b"indices_stride=63 not smaller than topk=64"),
  (dict(cache_seqlens=None), False, 1, b"cache_seqlens / indices / topk_lens must be non-NULL"),
  (dict(topk_lens=None), True, 1, b"cache_seqlens / indices / topk_lens must be non-NULL"),
  (dict(scores=2), False, 6, b"4-byte aligned"),
  (dict(block_table=2), True, 6, b"4-byte aligned"),
])
def test_the_statuses_and_their_order(lib, over, positions, status, text):
  p = _params(over, positions)
  assert lib.ffpa_attn_mla_sparse_topk_slots(ctypes.byref(p), None) == status, lib.ffpa_attn_last_error()
  assert text in lib.ffpa_attn_last_error(), lib.ffpa_attn_last_error()
  assert lib.ffpa_attn_mla_sparse_topk_slots(None, None) == 1


def test_page_size_is_not_looked_at_without_a_table_and_no_tokens_launch_nothing(lib):
  p = _params(dict(block_table=None, page_size=0, W=0, T=0))
  assert lib.ffpa_attn_mla_sparse_topk_slots(ctypes.byref(p), None) == 0, lib.ffpa_attn_last_error()


# ----------------------------------------------------------------------------- the argument errors of the two calls
def _good(T=6, N=40, B=2, W=3, device="cpu"):
  g = torch.Generator().manual_seed(0)
  return dict(scores=torch.randn(T, N, generator=g).to(device), positions=torch.randint(-1, N, (T, 8), generator=g, dtype=torch.int32).to(device),
              lens=torch.full((B,), N, dtype=torch.int32, device=device), table=torch.arange(B * W, dtype=torch.int32, device=device).view(B, W),
              cu=torch.tensor([0, 2, T], dtype=torch.int32, device=device))


def test_argument_errors_of_the_selection():
  a = _good()
  s, lens, table, cu = a["scores"], a["lens"], a["table"], a["cu"]
  with pytest.raises(TypeError, match="scores must be a tensor"):
    topk_slots(s.tolist(), 8, lens)
  with pytest.raises(TypeError, match="scores must be torch.float32, got torch.bfloat16 .bf16 / fp16 scores are not served"):
    topk_slots(s.bfloat16(), 8, lens)
  with pytest.raises(TypeError, match="cache_seqlens must be an int32 tensor"):
    topk_slots(s, 8, lens.long())
  with pytest.raises(TypeError, match="block_table must be an int32 tensor"):
    topk_slots(s, 8, lens, table.long(), 16)
  with pytest.raises(TypeError, match="cu_seqlens_q must be an int32 tensor"):
    topk_slots(s, 8, lens, cu_seqlens_q=cu.long())
  for bad in (8.0, True, None, torch.tensor(8)):
    with pytest.raises(TypeError, match="topk must be an int"):
      topk_slots(s, bad, lens)
  for bad in (None, 16.0, True):
    with pytest.raises(TypeError, match="page_size must be an int"):
      topk_slots(s, 8, lens, table, bad)
  with pytest.raises(NotImplementedError, match="inference only: scores requires grad"):
    topk_slots(s.clone().requires_grad_(), 8, lens)
  with torch.no_grad(), pytest.raises(NotImplementedError):  # (no grad mode: the next refusal is the CPU tensor's)
    topk_slots(s.clone().requires_grad_(), 8, lens)
  with pytest.raises(ValueError, match=r"scores must be \[T, N\]"):
    topk_slots(s[0], 8, lens)
  with pytest.raises(ValueError, match=r"scores must be \[T, N\]"):
    topk_slots(s[:, :0], 8, lens)
  for bad in (0, -1, 41):
    with pytest.raises(ValueError, match=r"topk must lie in \[1, N=40\]"):
      topk_slots(s, bad, lens)
  with pytest.raises(ValueError, match="contiguous last dimension"):
    topk_slots(s[:, ::2], 8, lens)
  with pytest.raises(ValueError, match=r"cache_seqlens must be an int32 tensor \[B\]"):
    topk_slots(s, 8, lens[None])
  with pytest.raises(ValueError, match=r"cache_seqlens must be an int32 tensor \[B\]"):
    topk_slots(s, 8, lens[:0])
  with pytest.raises(ValueError, match=r"cu_seqlens_q must be an int32 tensor \[B \+ 1 = 3\]"):
    topk_slots(s, 8, lens, cu_seqlens_q=cu[:2])
  with pytest.raises(ValueError, match="T must be a multiple of B=4"):
    topk_slots(s, 8, torch.zeros(4, dtype=torch.int32))
  for bad in (0, -16):
    with pytest.raises(ValueError, match="page_size must be a positive int"):
      topk_slots(s, 8, lens, table, bad)
  with pytest.raises(ValueError, match=r"block_table must be \[B=2, pages_per_seq >= 1\]"):
    topk_slots(s, 8, lens, table[:1], 16)
  with pytest.raises(ValueError, match=r"block_table must be \[B=2, pages_per_seq >= 1\]"):
    topk_slots(s, 8, lens, table[:, :0], 16)
  with pytest.raises(ValueError, match="block_table must have a contiguous last dimension"):
    topk_slots(s, 8, lens, table.t().contiguous().t(), 16)
  with pytest.raises(ValueError, match="cache_seqlens must be on scores's device"):
    topk_slots(s.to("meta"), 8, lens)
  # every argument right, on the CPU: there is no kernel for it
  with pytest.raises(NotImplementedError):
    topk_slots(s, 8, lens, table, 16, cu_seqlens_q=cu, causal=False)
  # a row stride is free, a padded table too: no refusal in front of the op
  with pytest.raises(NotImplementedError):
    topk_slots(torch.zeros(6, 64)[:, :40], 8, lens, torch.zeros(2, 8, dtype=torch.int32)[:, :3], 16)


def test_argument_errors_of_the_positions_mode():
  a = _good()
  pos, lens, table, cu = a["positions"], a["lens"], a["table"], a["cu"]
  with pytest.raises(TypeError, match="positions must be a tensor"):
    slots(None, lens)
  with pytest.raises(TypeError, match="positions must be torch.int32, got torch.int64"):
    slots(pos.long(), lens)
  with pytest.raises(TypeError, match="cache_seqlens must be an int32 tensor"):
    slots(pos, lens.float())
  with pytest.raises(TypeError, match="page_size must be an int"):
    slots(pos, lens, table)
  with pytest.raises(ValueError, match=r"positions must be \[T, topk\]"):
    slots(pos[0], lens)
  with pytest.raises(ValueError, match="contiguous last dimension"):
    slots(pos[:, ::2], lens)
  with pytest.raises(ValueError, match=r"cu_seqlens_q must be an int32 tensor \[B \+ 1 = 3\]"):
    slots(pos, lens, cu_seqlens_q=cu[None])
  with pytest.raises(ValueError, match="page_size must be a positive int"):
    slots(pos, lens, table, 0)
  with pytest.raises(ValueError, match="block_table must be on positions's device"):
    slots(pos, lens, table.to("meta"), 16)
  with pytest.raises(NotImplementedError):
    slots(pos, lens, table, 16, cu_seqlens_q=cu)


def test_no_tokens_return_empty_tensors_and_launch_nothing():
  lens = torch.zeros(2, dtype=torch.int32)
  idx, n = topk_slots(torch.zeros(0, 40), 8, lens)
  assert idx.shape == (0, 8) and idx.dtype == torch.int32 and n.shape == (0,) and n.dtype == torch.int32
  idx, n = slots(torch.zeros(0, 8, dtype=torch.int32), lens, cu_seqlens_q=torch.zeros(3, dtype=torch.int32))
  assert idx.shape == (0, 8) and idx.dtype == torch.int32 and n.shape == (0,) and n.dtype == torch.int32


# ----------------------------------------------------------------------------- the ops' fakes
def test_the_ops_have_fakes():
  from torch._subclasses.fake_tensor import FakeTensorMode

  with FakeTensorMode():
    s = torch.empty(12, 9000, device="cuda")[:, :8192]
    lens, cu = torch.empty(3, dtype=torch.int32, device="cuda"), torch.empty(4, dtype=torch.int32, device="cuda")
    table = torch.empty(3, 200, dtype=torch.int32, device="cuda")
    for idx, n in (topk_slots(s, 2048, lens, table, 64, cu_seqlens_q=cu), topk_slots(s, 100, lens), torch.ops.ffpa_attn._mla_sparse_topk_slots_hip(s, 7, lens, None, 1, None, False)):
      assert idx.shape == (12, idx.size(1)) and idx.size(1) in (2048, 100, 7) and idx.dtype == torch.int32 and idx.is_contiguous() and idx.device == s.device
      assert n.shape == (12,) and n.dtype == torch.int32 and n.device == s.device
    pos = torch.empty(12, 300, dtype=torch.int32, device="cuda")[:, :256]
    for idx, n in (slots(pos, lens, table, 16), torch.ops.ffpa_attn._mla_sparse_slots_hip(pos, lens, None, 1, cu)):
      assert idx.shape == (12, 256) and idx.dtype == torch.int32 and idx.is_contiguous() and n.shape == (12,) and n.dtype == torch.int32


def test_a_step_with_the_selection_compiles_on_meta_tensors():
  q = torch.empty(12, 128, 576, dtype=torch.bfloat16, device="meta")
  pool = torch.empty(40, 64, 1, 576, dtype=torch.bfloat16, device="meta")
  i32 = lambda *s: torch.empty(s, dtype=torch.int32, device="meta")

  def f(q, pool, scores, lens, table):
    idx, n = ffpa_attn_amd.ffpa_mla_sparse_topk_slots(scores, 320, lens, table, 64)
    return ffpa_attn_amd.ffpa_attn_with_kvcache_mla_sparse(q, pool, 512, idx, topk_lens=n, softmax_scale=0.07) * 2, n

  args = (q, pool, torch.empty(12, 2560, device="meta"), i32(3), i32(3, 40))
  for fn in (f, torch.compile(f, fullgraph=True, backend="eager")):
    out, n = fn(*args)
    assert out.shape == (12, 128, 512) and out.dtype == torch.bfloat16 and out.device.type == "meta" and n.shape == (12,) and n.dtype == torch.int32


# ----------------------------------------------------------------------------- the definition against brute force
VALUES = (-1.0, -0.0, 0.0, 1.0, float("nan"))
ORDER = (0, 1, 1, 2, 3)  # the rank of each value in the selection's order: -0.0 with +0.0, NaN on top


@pytest.mark.parametrize("N", range(1, 8))
def test_the_reference_selects_what_brute_force_selects(N):
  """Every row of N <= 7 columns over {-1, -0.0, 0.0, 1, NaN}, every topk <= 7.  Brute force, with no sort in it: position p is selected iff fewer than topk
  positions beat it — hold a larger value, or an equal one at a lower position."""
  codes = np.array(list(itertools.product(range(5), repeat=N)), dtype=np.int64)  # [5^N, N]
  rows = torch.tensor(VALUES, dtype=torch.float32)[torch.from_numpy(codes)]
  assert torch.equal(torch.signbit(rows), torch.from_numpy(np.isin(codes, (0, 1))))  # (the -0.0 made it into the tensor)
  key = np.array(ORDER)[codes]
  for topk in range(1, 8):
    for n in range(N + 1):  # the visible length: columns at and past it never count, whatever they hold
      got = TR.select(rows, n, topk)
      want_mask = beaten_by(key, n) < topk
      assert got.shape == (len(codes), min(n, topk))
      got_mask = np.zeros_like(want_mask)
      np.put_along_axis(got_mask, got.numpy(), True, axis=1)
      assert (got_mask == want_mask).all() and (np.diff(got.numpy(), axis=1) > 0).all()


def beaten_by(key, n):
  """Per (row, position p): how many of the first n positions beat p; a p at or past n is beaten by more than any topk."""
  k = key[:, :n]
  beats = (k[:, :, None] > k[:, None, :]) | ((k[:, :, None] == k[:, None, :]) & (np.arange(n)[:, None] < np.arange(n)[None, :]))  # [row, q, p]: q beats p
  out = np.full(key.shape, 1 << 20, dtype=np.int64)
  out[:, :n] = beats.sum(axis=1)
  return out


def test_the_reference_end_to_end_on_a_small_ragged_step():
  """Lengths, causal alignment, padding rows, translation and tail, worked by hand."""
  scores = torch.tensor([[5., 1., 9., 9., 0., 7.]] * 5)
  scores[4] = float("nan")
  lens, cu = torch.tensor([4, 6], dtype=torch.int32), torch.tensor([0, 1, 4], dtype=torch.int32)
  table = torch.tensor([[7, 3, 0], [2, 9, 4]], dtype=torch.int32)
  # rows: seq 0 token 0 of 1 (n = 4); seq 1 tokens 0 .. 2 of 3 (n = 4, 5, 6 causal; 6 otherwise); row 4: padding
  idx, n = TR.topk_slots(scores, 3, lens, cu_seqlens_q=cu)
  assert n.tolist() == [3, 3, 3, 3, 0]
  assert idx.tolist() == [[0, 2, 3], [0, 2, 3], [0, 2, 3], [2, 3, 5], [-1, -1, -1]]
  idx, n = TR.topk_slots(scores, 3, lens, cu_seqlens_q=cu, causal=False)
  assert idx.tolist() == [[0, 2, 3], [2, 3, 5], [2, 3, 5], [2, 3, 5], [-1, -1, -1]]
  idx, n = TR.topk_slots(scores, 5, lens, table, 2, cu_seqlens_q=cu)
  assert n.tolist() == [4, 4, 5, 5, 0]
  assert idx.tolist() == [[14, 15, 6, 7, -1], [4, 5, 18, 19, -1], [4, 5, 18, 19, 8], [4, 5, 18, 19, 9], [-1] * 5]
  # uniform [B, Sq] rows: token t % Sq of sequence t // Sq; a table shorter than the positions reads its last column
  idx, n = TR.topk_slots(scores[:4], 6, torch.tensor([2, 6], dtype=torch.int32), table[:, :2], 2)
  assert n.tolist() == [1, 2, 5, 6] and idx[3].tolist() == [4, 5, 18, 19, 18, 19] and idx[1].tolist() == [14, 15, -1, -1, -1, -1]


# ----------------------------------------------------------------------------- the definition's positions mode against the two torch helpers
@pytest.mark.parametrize("page_size, ragged", [(1, False), (16, True), (64, False), (48, True)])
def test_the_references_positions_mode_is_the_two_helpers_composed(page_size, ragged):
  g = torch.Generator().manual_seed(page_size)
  B, T, topk, W = 3, 12, 50, 9
  cu = torch.tensor([0, 5, 5, 11], dtype=torch.int32) if ragged else None  # (row 11: padding)
  seq = torch.tensor([0] * 5 + [2] * 6 + [0] if ragged else [t // 4 for t in range(T)])
  positions = torch.randint(0, W * page_size + 5, (T, topk), generator=g, dtype=torch.int32)  # (some reach past the table: its last column)
  positions[torch.rand(T, topk, generator=g) < 0.3] = -1
  positions[1], positions[2, :20], positions[3, 10:] = -1, -1, -7
  table = torch.randperm(B * W, generator=g).to(torch.int32).view(B, W)
  lens = torch.full((B,), 10 ** 6, dtype=torch.int32)
  got_idx, got_n = TR.slots(positions, lens, table, page_size, cu_seqlens_q=cu)
  want_idx, want_n = ffpa_attn_amd.compact_topk_indices(ffpa_attn_amd.slots_from_block_table(positions, table[seq], page_size))
  live = slice(0, 11) if ragged else slice(0, T)
  assert torch.equal(got_n[live], want_n[live]) and got_n.dtype == torch.int32 and got_idx.dtype == torch.int32
  front = torch.arange(topk)[None] < got_n[:, None]
  assert torch.equal(got_idx[live][front[live]], want_idx[live][front[live]]) and (got_idx[~front] == -1).all()
  if ragged:
    assert got_n[11] == 0 and (got_idx[11] == -1).all()
  none_idx, none_n = TR.slots(positions, lens, cu_seqlens_q=cu)
  want_idx, _ = ffpa_attn_amd.compact_topk_indices(positions)
  assert torch.equal(none_n, got_n) and torch.equal(none_idx[live][front[live]], want_idx[live][front[live]])
