"""The paged-KV call without a GPU: the C struct against its ctypes mirror, every argument check of ffpa_attn_varlen_paged_fwd (they come before
any device work), its launch plan next to the packed call's, and the public ffpa_attn_with_kvcache's refusals on meta tensors."""

import ctypes
import os
import subprocess

import pytest
import torch

from ffpa_attn_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
  if not hip.library_available():
    from ffpa_attn_amd import build

    build.build()
  return hip.load_library()


def _params(**over):
  p = hip.FfpaVarlenFwdParams()
  p.struct_size = ctypes.sizeof(hip.FfpaVarlenFwdParams)
  p.abi_version = hip.ABI_VERSION
  buf = (ctypes.c_char * 4096)()
  base = (ctypes.addressof(buf) + 15) & ~15
  p.q = p.k = p.v = p.o = base
  p.cu_seqlens_q = p.seqused_kv = base
  p.cu_seqlens_kv = None
  p.batch, p.heads_q, p.heads_kv, p.head_dim = 3, 8, 2, 512
  p.max_seqlen_q, p.max_seqlen_kv = 1000, 2000
  p.q_stride[:] = [8 * 512, 512]
  p.k_stride[:] = [2 * 512, 512]
  p.v_stride[:] = [2 * 512, 512]
  p.o_stride[:] = [8 * 512, 512]
  p.dtype, p.causal = 0, 1
  p.softmax_scale, p.rescale_threshold = 512 ** -0.5, -1.0
  for name, value in over.items():
    if name.endswith("_stride"):
      getattr(p, name)[:] = value
    else:
      setattr(p, name, value)
  p._keepalive = buf
  return p


def _kv(p, **over):
  kv = hip.FfpaPagedKv()
  kv.struct_size = ctypes.sizeof(hip.FfpaPagedKv)
  kv.block_table = p.q
  kv.pages_per_row, kv.page_size, kv.num_pages = 32, 64, 96
  kv.bt_stride = 32
  kv.k_page_stride = kv.v_page_stride = 64 * 2 * 512
  for name, value in over.items():
    setattr(kv, name, value)
  return kv


def test_ctypes_mirror_of_the_paged_kv_matches_the_c_header(tmp_path):
  fields = [f[0] for f in hip.FfpaPagedKv._fields_]
  src = tmp_path / "layout.c"
  body = "".join(f'printf("{f} %zu\\n", offsetof(ffpa_paged_kv, {f}));\n' for f in fields)
  src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ffpa_attn.h"\nint main(void){\n'
                 'printf("sizeof %zu\\n", sizeof(ffpa_paged_kv));\n' + body + "return 0;}\n")
  exe = tmp_path / "layout"
  subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
  out = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
  assert int(out["sizeof"]) == ctypes.sizeof(hip.FfpaPagedKv) == 56
  for f in fields:
    assert int(out[f]) == getattr(hip.FfpaPagedKv, f).offset, f


def test_abi_version_and_exports(lib):
  assert hip.ABI_VERSION == 7 and lib.ffpa_attn_query(0) == 7
  for name in ("ffpa_attn_varlen_paged_fwd", "ffpa_attn_varlen_paged_fwd_plan", "ffpa_attn_varlen_paged_fwd_kernel", "ffpa_attn_varlen_paged_fwd_workspace_bytes"):
    assert name in hip.EXPORTS and getattr(lib, name) is not None


@pytest.mark.parametrize("p_over, kv_over, status, text", [
  (dict(), dict(page_size=32), 4, b"page_size"),
  (dict(), dict(page_size=96), 4, b"page_size"),
  (dict(), dict(page_size=0), 4, b"page_size"),
  (dict(), dict(block_table=None), 1, b"block_table"),
  (dict(seqused_kv=None), dict(), 1, b"seqused_kv"),
  (dict(), dict(k_page_stride=-8), 5, b"negative"),
  (dict(), dict(v_page_stride=64 * 2 * 512 + 4), 5, b"multiple of 8"),
  (dict(), dict(bt_stride=16), 5, b"bt_stride"),
  (dict(), dict(num_pages=0), 4, b"num_pages"),
  (dict(), dict(pages_per_row=0), 4, b"pages_per_row"),
  (dict(), dict(struct_size=48), 10, b"ffpa_paged_kv ABI mismatch"),
  (dict(abi_version=6), dict(), 10, b"ABI mismatch"),
  (dict(head_dim=100), dict(), 3, b"headdim not support"),
  (dict(k_stride=[256, 512]), dict(), 5, b"rows must not overlap"),
  (dict(q=0), dict(), 1, b"non-NULL"),
])
def test_status_codes_of_the_paged_call_come_before_any_device_work(lib, p_over, kv_over, status, text):
  p = _params(**p_over)
  kv = _kv(p, **kv_over)
  assert lib.ffpa_attn_varlen_paged_fwd(ctypes.byref(p), ctypes.byref(kv), None) == status
  assert text in lib.ffpa_attn_last_error(), lib.ffpa_attn_last_error()


def test_misaligned_pointers_of_the_paged_call(lib):
  p = _params()
  kv = _kv(p, block_table=p.q + 2)
  assert lib.ffpa_attn_varlen_paged_fwd(ctypes.byref(p), ctypes.byref(kv), None) == 6
  p = _params()
  p.seqused_kv = p.seqused_kv + 2
  assert lib.ffpa_attn_varlen_paged_fwd(ctypes.byref(p), ctypes.byref(_kv(p)), None) == 6
  p = _params()
  p.k = p.k + 8
  assert lib.ffpa_attn_varlen_paged_fwd(ctypes.byref(p), ctypes.byref(_kv(p)), None) == 6
  assert lib.ffpa_attn_varlen_paged_fwd(ctypes.byref(p), None, None) == 1
  assert lib.ffpa_attn_varlen_paged_fwd(None, ctypes.byref(_kv(p)), None) == 1


def test_contiguous_call_still_wants_cu_seqlens_kv(lib):
  # (the paged call ignores cu_seqlens_kv; the packed call keeps requiring it)
  p = _params()
  assert lib.ffpa_attn_varlen_fwd(ctypes.byref(p), None) == 1 and b"cu_seqlens" in lib.ffpa_attn_last_error()


@pytest.mark.parametrize("d", [128, 192, 200, 256, 320, 384, 512, 576, 640, 1024])
@pytest.mark.parametrize("shape", [dict(max_seqlen_q=1, heads_q=32, heads_kv=8, batch=32, max_seqlen_kv=16384), dict(max_seqlen_q=1000, batch=3),
                                   dict(max_seqlen_q=4, heads_q=32, heads_kv=8, batch=16, max_seqlen_kv=4096)])
def test_paged_plan_against_the_contiguous_plan(lib, d, shape):
  dk = (d + 63) // 64 * 64
  over = dict(shape, head_dim=d, total_q=shape["batch"] * shape["max_seqlen_q"])
  over["k_stride"] = over["v_stride"] = [over.get("heads_kv", 2) * d, d]
  over["q_stride"] = over["o_stride"] = [over.get("heads_q", 8) * d, d]
  p = _params(**over)
  p.cu_seqlens_kv = p.q
  p.workspace, p.workspace_bytes = p.q, 1 << 40
  kv = _kv(p, k_page_stride=64 * over["k_stride"][0], v_page_stride=64 * over["k_stride"][0])
  want, got = (ctypes.c_int * 5)(), (ctypes.c_int * 5)()
  assert lib.ffpa_attn_varlen_fwd_plan(ctypes.byref(p), want) == 0, lib.ffpa_attn_last_error()
  assert lib.ffpa_attn_varlen_paged_fwd_plan(ctypes.byref(p), ctypes.byref(kv), got) == 0, lib.ffpa_attn_last_error()
  bc = 32 if dk > 512 else 64
  assert got[2] == bc
  if dk in (256, 320):
    assert want[2] == 128  # (the packed call's 128-key tile: the paged call takes 64)
  else:
    assert list(got) == list(want), (list(got), list(want))
  assert got[:2] == want[:2]
  name = ctypes.create_string_buffer(200)
  assert lib.ffpa_attn_varlen_paged_fwd_kernel(ctypes.byref(p), ctypes.byref(kv), name, len(name)) == 0
  assert name.value.decode().startswith(f"ffpa_fwd_m16_paged_kernel<bf16, {dk}")
  assert name.value.decode().endswith("+ ffpa_varlen_merge_kernel") == (got[4] > 1)
  # the scratch the paged call asks for is sized by its own plan
  ws = lib.ffpa_attn_varlen_paged_fwd_workspace_bytes(ctypes.byref(p), ctypes.byref(kv))
  assert (ws > 0) == (got[4] > 1)
  # and the Python side asks the same question
  plan = hip.varlen_launch_plan(p.batch, p.heads_q, p.heads_kv, p.max_seqlen_q, p.max_seqlen_kv, d, total_q=p.total_q, page_size=64)
  assert plan["block_keys"] == bc and plan["kernel"].startswith("ffpa_fwd_m16_paged_kernel")


# ---- the public call on meta tensors: everything it refuses, it refuses before touching a device
def _meta(*shape, dtype=torch.bfloat16):
  return torch.empty(*shape, dtype=dtype, device="meta")


@pytest.mark.parametrize("kw, name", [
  (dict(k=_meta(2, 1, 8, 128)), "k"),
  (dict(v=_meta(2, 1, 8, 128)), "v"),
  (dict(rotary_cos=_meta(64, 32)), "rotary_cos"),
  (dict(rotary_sin=_meta(64, 32)), "rotary_sin"),
  (dict(cache_batch_idx=_meta(2, dtype=torch.int32)), "cache_batch_idx"),
  (dict(cache_leftpad=_meta(2, dtype=torch.int32)), "cache_leftpad"),
  (dict(window_size=(128, 0)), "window_size"),
  (dict(softcap=30.0), "softcap"),
  (dict(alibi_slopes=_meta(32, dtype=torch.float32)), "alibi_slopes"),
])
def test_with_kvcache_names_what_it_does_not_implement(kw, name):
  from ffpa_attn_amd import ffpa_attn_with_kvcache

  q, kc = _meta(2, 1, 32, 128), _meta(2, 256, 8, 128)
  with pytest.raises(NotImplementedError, match=name):
    ffpa_attn_with_kvcache(q, kc, kc, cache_seqlens=10, **kw)


def test_with_kvcache_refusals():
  import ffpa_attn_amd
  from ffpa_attn_amd import ffpa_attn_with_kvcache

  assert "ffpa_attn_with_kvcache" in ffpa_attn_amd.__all__
  q, kc = _meta(2, 1, 32, 128), _meta(2, 256, 8, 128)
  with pytest.raises(TypeError, match="fp16/bf16"):
    ffpa_attn_with_kvcache(q.float(), kc, kc)
  with pytest.raises(TypeError, match="fp16/bf16"):
    ffpa_attn_with_kvcache(q, kc.half(), kc.half())
  with pytest.raises(TypeError, match="cache_seqlens"):
    ffpa_attn_with_kvcache(q, kc, kc, cache_seqlens=3.0)
  with pytest.raises(ValueError, match="cache_seqlens"):
    ffpa_attn_with_kvcache(q, kc, kc, cache_seqlens=_meta(2, dtype=torch.int64))
  with pytest.raises(ValueError, match="num_heads"):
    ffpa_attn_with_kvcache(_meta(2, 1, 30, 128), kc, kc)
  with pytest.raises(ValueError, match="head dim"):
    ffpa_attn_with_kvcache(_meta(2, 1, 32, 64), kc, kc)
  with pytest.raises(ValueError, match="share their shape"):
    ffpa_attn_with_kvcache(q, kc, _meta(2, 128, 8, 128))
  with pytest.raises(ValueError, match="batch"):
    ffpa_attn_with_kvcache(q, _meta(3, 256, 8, 128), _meta(3, 256, 8, 128))
  # paged: page size, table type / shape
  bt = _meta(2, 4, dtype=torch.int32)
  with pytest.raises(ValueError, match="page_size"):
    ffpa_attn_with_kvcache(q, _meta(16, 32, 8, 128), _meta(16, 32, 8, 128), cache_seqlens=10, block_table=bt)
  with pytest.raises(ValueError, match="page_size"):
    ffpa_attn_with_kvcache(q, _meta(16, 96, 8, 128), _meta(16, 96, 8, 128), cache_seqlens=10, block_table=bt)
  with pytest.raises(ValueError, match="block_table"):
    ffpa_attn_with_kvcache(q, _meta(16, 64, 8, 128), _meta(16, 64, 8, 128), cache_seqlens=10, block_table=_meta(2, 4, dtype=torch.int64))
  with pytest.raises(ValueError, match="block_table"):
    ffpa_attn_with_kvcache(q, _meta(16, 64, 8, 128), _meta(16, 64, 8, 128), cache_seqlens=10, block_table=_meta(3, 4, dtype=torch.int32))
  # inference only: a tensor that requires grad raises instead of returning an output with no gradient
  qg = torch.empty(2, 1, 32, 128, dtype=torch.bfloat16, device="meta", requires_grad=True)
  with pytest.raises(NotImplementedError, match="inference only"):
    ffpa_attn_with_kvcache(qg, kc, kc, cache_seqlens=10)


def test_with_kvcache_paged_shapes_on_meta():
  # the paged route runs the registered op's fake on meta tensors: output [B, Sq, Hq, D], LSE [B, Hq, Sq]
  from ffpa_attn_amd import ffpa_attn_with_kvcache

  q = _meta(3, 4, 32, 512)
  pool = _meta(40, 128, 8, 512)
  bt = _meta(3, 5, dtype=torch.int32)
  out, lse = ffpa_attn_with_kvcache(q, pool, pool, cache_seqlens=_meta(3, dtype=torch.int32), block_table=bt, causal=True, return_softmax_lse=True)
  assert out.shape == (3, 4, 32, 512) and out.dtype == torch.bfloat16
  assert lse.shape == (3, 32, 4) and lse.dtype == torch.float32


def test_packed_entry_points_still_reject_block_table():
  # (the reference's contract for ffpa_attn_varlen_func: the paged cache has its own entry point)
  import ffpa_attn_amd

  q = torch.empty(10, 2, 512, dtype=torch.bfloat16, device="meta")
  cu = torch.tensor([0, 4, 10], dtype=torch.int32)
  with pytest.raises(NotImplementedError, match="block_table"):
    ffpa_attn_amd.ffpa_attn_varlen_func(q, q, q, cu, cu, 6, 6, block_table=torch.zeros(2, 1, dtype=torch.int32))
