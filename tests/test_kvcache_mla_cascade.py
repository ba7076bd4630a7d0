"""Shared-prefix (cascade) attention over the MLA latent cache without a GPU: the public names, the plan entry point in the header and in hip.EXPORTS, the ABI
pin, the ctypes mirror of ffpa_mla_cascade_plan_params against gcc, every refusal of ffpa_attn_mla_cascade_plan (they come before any device work), the refusals
of the two front ends (their own, and every rule of _mla_check under the new names), the fakes on meta tensors, cascade=None, and the torch restatement of the
plan (tests/kvcache_mla_cascade_ref.py) on hand-worked cases."""

import ctypes
import inspect
import json
import os
import re
import subprocess

import pytest
import torch

import ffpa_attn_amd
from ffpa_attn_amd import hip
from ffpa_attn_amd.kvcache import mla_cascade_rule

from kvcache_mla_cascade_ref import plan as ref_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALE = 192 ** -0.5
CALLS = ("ffpa_attn_with_kvcache_mla_cascade", "ffpa_attn_with_kvcache_mla_cascade_fp8")


@pytest.fixture(scope="module")
def lib():
  if not hip.library_available():
    from ffpa_attn_amd import build

    build.build()
  return hip.load_library()


def test_public_names():
  for name in CALLS + ("mla_cascade_rule",):
    assert name in ffpa_attn_amd.__all__ and callable(getattr(ffpa_attn_amd, name)), name


def test_abi_version_stays_7_and_the_symbol_is_declared_and_exported(lib):
  assert hip.ABI_VERSION == 7 and lib.ffpa_attn_query(0) == 7
  assert "ffpa_attn_mla_cascade_plan" in hip.EXPORTS and lib.ffpa_attn_mla_cascade_plan is not None
  header = open(os.path.join(ROOT, "include", "ffpa_attn.h")).read()
  declared = set(re.findall(r"^\s*(?:int|size_t|const char\*)\s+(ffpa_attn_\w+)\s*\(", header, flags=re.M))
  assert "ffpa_attn_mla_cascade_plan" in declared and declared == set(hip.EXPORTS)
  assert hip.MLA_BUILDS == ((576, 512),)


def test_ctypes_mirror_of_the_plan_params_matches_the_c_header(tmp_path):
  fields = [f[0] for f in hip.FfpaMlaCascadePlanParams._fields_]
  src = tmp_path / "layout.c"
  body = "".join(f'printf("{f} %zu\\n", offsetof(ffpa_mla_cascade_plan_params, {f}));\n' for f in fields)
  src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ffpa_attn.h"\nint main(void){\n'
                 'printf("sizeof %zu\\n", sizeof(ffpa_mla_cascade_plan_params));\n'
                 'printf("merge %zu\\n", sizeof(ffpa_merge_states_params));\nprintf("varlen %zu\\n", sizeof(ffpa_varlen_fwd_params));\n'
                 'printf("paged %zu\\n", sizeof(ffpa_paged_kv));\nprintf("abi %d\\n", FFPA_ATTN_ABI_VERSION);\n' + body + "return 0;}\n")
  exe = tmp_path / "layout"
  subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
  out = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
  assert int(out["sizeof"]) == ctypes.sizeof(hip.FfpaMlaCascadePlanParams) == 120
  for f in fields:
    assert int(out[f]) == getattr(hip.FfpaMlaCascadePlanParams, f).offset, f
  # the existing layouts and the ABI version stay where they were
  assert int(out["merge"]) == 144 and int(out["varlen"]) == 216 and int(out["paged"]) == 56 and int(out["abi"]) == 7


# ---- the C entry point: every refusal comes before any device work, so host buffers will do
B_, G_, W_ = 6, 3, 5


def _params(**over):
  """A well-formed plan (6 sequences in 3 groups, 5 pages of 64 rows per sequence, Sq 2, causal) over one host buffer: each test breaks one argument."""
  p = hip.FfpaMlaCascadePlanParams()
  p.struct_size = ctypes.sizeof(hip.FfpaMlaCascadePlanParams)
  p.abi_version = hip.ABI_VERSION
  buf = (ctypes.c_char * 4096)()
  base = (ctypes.addressof(buf) + 15) & ~15
  off = 0
  for name, n in (("cu_group_seqs", G_ + 1), ("shared_prefix_len", G_), ("lens", B_), ("block_table", B_ * W_), ("cu_q_prefix", G_ + 1), ("prefix_lens", G_),
                  ("prefix_table", G_ * W_), ("suffix_table", B_ * W_), ("suffix_lens", B_)):
    setattr(p, name, base + off)
    off += 4 * n
  p.bt_stride = W_
  p.batch, p.groups, p.pages_per_seq, p.page_size, p.seqlen_q, p.causal, p.capacity, p.shared_prefix_len_host = B_, G_, W_, 64, 2, 1, W_ * 64, 0
  for name, value in over.items():
    setattr(p, name, value(p) if callable(value) else value)
  p._keepalive = buf
  return p


@pytest.mark.parametrize("over, status, text", [
  (dict(struct_size=112), 10, b"ffpa_mla_cascade_plan_params ABI mismatch"),
  (dict(abi_version=6), 10, b"ABI mismatch"),
  (dict(lens=None), 1, b"lens"),
  (dict(block_table=None), 1, b"block_table"),
  (dict(cu_q_prefix=None), 1, b"cu_q_prefix"),
  (dict(prefix_lens=None), 1, b"prefix_lens"),
  (dict(prefix_table=None), 1, b"prefix_table"),
  (dict(suffix_table=None), 1, b"suffix_table"),
  (dict(suffix_lens=None), 1, b"suffix_lens"),
  (dict(batch=0), 4, b"batch=0"),
  (dict(pages_per_seq=0), 4, b"pages_per_seq=0"),
  (dict(groups=0), 4, b"groups=0 must be at least 1"),
  (dict(groups=-1), 4, b"at least 1"),
  (dict(cu_group_seqs=None), 4, b"without cu_group_seqs"),
  (dict(seqlen_q=0), 4, b"seqlen_q=0"),
  (dict(seqlen_q=2 ** 30), 4, b"2^31"),
  (dict(page_size=0), 4, b"page_size=0"),
  (dict(page_size=96), 4, b"multiple of 64"),
  (dict(page_size=-64), 4, b"multiple of 64"),
  (dict(causal=2), 4, b"causal=2"),
  (dict(capacity=0), 4, b"capacity=0"),
  (dict(capacity=W_ * 64 + 1), 4, b"capacity"),
  (dict(shared_prefix_len=None, shared_prefix_len_host=-1), 4, b"negative"),
  (dict(bt_stride=W_ - 1), 5, b"row stride"),
  (dict(lens=lambda p: p.lens + 2), 6, b"lens must be 4-byte aligned"),
  (dict(suffix_lens=lambda p: p.suffix_lens + 1), 6, b"aligned"),
  (dict(cu_group_seqs=lambda p: p.cu_group_seqs + 3), 6, b"cu_group_seqs"),
  # an output on an input, on the tail of an input, and on another output
  (dict(suffix_lens=lambda p: p.lens), 4, b"suffix_lens overlaps lens"),
  (dict(prefix_lens=lambda p: p.shared_prefix_len), 4, b"overlap"),
  (dict(cu_q_prefix=lambda p: p.cu_group_seqs), 4, b"overlap"),
  (dict(suffix_table=lambda p: p.block_table + 4 * (B_ * W_ - 1)), 4, b"suffix_table overlaps block_table"),
  (dict(prefix_table=lambda p: p.suffix_table), 4, b"overlap"),
  (dict(suffix_lens=lambda p: p.suffix_table + 4 * (B_ * W_ - 1)), 4, b"overlap"),
  (dict(bt_stride=W_ + 1), 4, b"overlaps block_table"),  # (a wider input table now reaches into the first output)
])
def test_status_codes_of_the_plan_come_before_any_device_work(lib, over, status, text):
  p = _params(**over)
  assert lib.ffpa_attn_mla_cascade_plan(ctypes.byref(p), None) == status, lib.ffpa_attn_last_error()
  assert text in lib.ffpa_attn_last_error(), lib.ffpa_attn_last_error()


def test_a_null_params_pointer(lib):
  assert lib.ffpa_attn_mla_cascade_plan(None, None) == 1


# ---- the front ends: everything they refuse, they refuse before touching a device
def _meta(*shape, dtype=torch.bfloat16):
  return torch.empty(*shape, dtype=dtype, device="meta")


def _i32(*shape):
  return _meta(*shape, dtype=torch.int32)


def _call(name, **kw):
  fp8 = name.endswith("_fp8")
  args = dict(q=_meta(6, 1, 16, 576), kv_cache=_meta(40, 64, 1, 576, dtype=torch.float8_e4m3fn if fp8 else torch.bfloat16), head_dim_v=512,
              shared_prefix_len=128, cache_seqlens=_i32(6), block_table=_i32(6, 5), softmax_scale=SCALE)
  args.update(kw)
  q, pool, dv = args.pop("q"), args.pop("kv_cache"), args.pop("head_dim_v")
  return getattr(ffpa_attn_amd, name)(q, pool, dv, **args)


_OWN_REFUSALS = [
  (dict(block_table=None, kv_cache=_meta(6, 128, 1, 576)), ValueError, "block_table is required"),
  (dict(shared_prefix_len=True), TypeError, "shared_prefix_len must be an int or an int32 device tensor"),
  (dict(shared_prefix_len=64.0), TypeError, "shared_prefix_len must be an int or an int32 device tensor"),
  (dict(shared_prefix_len=None), TypeError, "shared_prefix_len must be"),
  (dict(shared_prefix_len=-64), ValueError, "non-negative"),
  (dict(shared_prefix_len=_meta(1, dtype=torch.int64)), TypeError, "must be int32"),
  (dict(shared_prefix_len=_i32(2)), ValueError, r"must be \[groups=1\]"),
  (dict(shared_prefix_len=_i32(1, 1)), ValueError, r"must be \[groups=1\]"),
  (dict(shared_prefix_len=torch.zeros(1, dtype=torch.int32)), ValueError, "on q's device"),
  (dict(shared_prefix_len=_i32(2), cu_group_seqs=_i32(4)), ValueError, r"must be \[groups=3\]"),
  (dict(cu_group_seqs=_meta(4, dtype=torch.int64)), TypeError, "cu_group_seqs must be an int32 tensor"),
  (dict(cu_group_seqs=[0, 3, 6]), TypeError, "cu_group_seqs must be an int32 tensor"),
  (dict(cu_group_seqs=_i32(1)), ValueError, r"\[groups \+ 1\]"),
  (dict(cu_group_seqs=_i32(2, 2)), ValueError, r"\[groups \+ 1\]"),
  (dict(cu_group_seqs=torch.zeros(4, dtype=torch.int32)), ValueError, "on q's device"),
  (dict(max_group_seqs=0), ValueError, "max_group_seqs"),
  (dict(max_group_seqs=2.0), ValueError, "max_group_seqs"),
  (dict(cascade=1), TypeError, "cascade must be True, False or None"),
  (dict(cascade="auto"), TypeError, "cascade must be"),
]

# every rule of _mla_check, under the new names
_MLA_CHECK_REFUSALS = [
  (dict(softmax_scale=None), TypeError, "softmax_scale is required"),
  (dict(softmax_scale="0.07"), TypeError, "real number"),
  (dict(q=None), TypeError, "q must be a tensor"),
  (dict(kv=_meta(6, 1, 1, 576).requires_grad_(True)), NotImplementedError, "inference only: kv requires grad"),
  (dict(q=_meta(6, 1, 16, 576, dtype=torch.float32)), TypeError, "fp16/bf16"),
  (dict(q=_meta(6, 16, 576)), ValueError, r"q must be \[B, Sq, Hq, D\]"),
  (dict(q=_meta(6, 1, 16, 512)), ValueError, "head dim of the cache"),
  (dict(head_dim_v=512.0), TypeError, "head_dim_v must be an int"),
  (dict(head_dim_v=500), ValueError, "multiples of 64"),
  (dict(head_dim_v=448), NotImplementedError, r"\(576, 448\) is not built"),
  (dict(q=_meta(6, 1, 5, 576), kv_cache=None), ValueError, "multiple of the latent num_heads"),  # (kv_cache: two latent heads, filled in below)
  (dict(num_splits=-1), ValueError, "num_splits"),
  (dict(kv_cache=None, q=_meta(6, 1, 16, 576, dtype=torch.float16)), TypeError, "fp16/bf16"),  # (a 16-bit pool of another dtype / a wrong FP8 format, below)
  (dict(block_table=_meta(6, 5, dtype=torch.int64)), ValueError, "block_table must be an int32 tensor"),
  (dict(block_table=_i32(5, 5)), ValueError, "block_table must be an int32 tensor"),
  (dict(block_table=_i32(6, 0)), ValueError, "at least one page"),
  (dict(block_table=torch.zeros(6, 5, dtype=torch.int32)), ValueError, "block_table must be on q's device"),
  (dict(cache_seqlens=-1), ValueError, "cache_seqlens must be non-negative"),
  (dict(cache_seqlens=2.0), TypeError, "cache_seqlens must be an int or an int32 tensor"),
  (dict(cache_seqlens=_i32(5)), ValueError, "cache_seqlens must be an int or an int32 tensor"),
  (dict(kv=_meta(6, 1, 1, 576, dtype=torch.float32)), TypeError, "kv must have"),
  (dict(kv=_meta(6, 1, 2, 576)), ValueError, r"kv must be \[B=6, Snew, Hkv=1, D=576\]"),
]


@pytest.mark.parametrize("name", CALLS)
@pytest.mark.parametrize("kw, exc, text, mode", [(kw, exc, text, mode) for kw, exc, text in _OWN_REFUSALS + _MLA_CHECK_REFUSALS for mode in (None, True, False)
                                                 if not ("cascade" in kw and mode is not None)])
def test_front_end_refusals_on_every_route(name, kw, exc, text, mode):
  fp8 = name.endswith("_fp8")
  kw = dict(kw)
  if "kv_cache" in kw and kw["kv_cache"] is None:  # (the two rows that need a pool of their own per family)
    if "multiple" in text:
      kw["kv_cache"] = _meta(40, 64, 2, 576, dtype=torch.float8_e4m3fn if fp8 else torch.bfloat16)
    else:
      kw["kv_cache"] = _meta(40, 64, 1, 576, dtype=torch.float8_e5m2 if fp8 else torch.bfloat16)
  if "kv_cache" in kw and kw.get("block_table", 0) is None and fp8:
    kw["kv_cache"] = kw["kv_cache"].to(torch.float8_e4m3fn)
  with pytest.raises(exc, match=text) as info:
    _call(name, **{"cascade": mode, **kw})
  assert str(info.value).startswith(name) or "softmax_scale" in kw, info.value


def test_page_size_and_missing_arguments():
  for name in CALLS:
    dtype = torch.float8_e4m3fn if name.endswith("_fp8") else torch.bfloat16
    with pytest.raises(ValueError, match="page_size .96. must be a positive multiple of 64"):
      _call(name, kv_cache=_meta(40, 96, 1, 576, dtype=dtype))
    fn = getattr(ffpa_attn_amd, name)
    q, pool = _meta(6, 1, 16, 576), _meta(40, 64, 1, 576, dtype=dtype)
    for drop in ("shared_prefix_len", "cache_seqlens", "block_table", "softmax_scale"):  # (required keywords)
      kw = dict(shared_prefix_len=128, cache_seqlens=_i32(6), block_table=_i32(6, 5), softmax_scale=SCALE)
      del kw[drop]
      with pytest.raises(TypeError, match=drop):
        fn(q, pool, 512, **kw)
  with pytest.raises(TypeError, match="kv_scale must be a host float"):
    _call(CALLS[1], kv_scale=torch.ones(()))
  with pytest.raises(ValueError, match="kv_scale must be finite"):
    _call(CALLS[1], kv_scale=0.0)


def test_signatures():
  want = ["q", "kv_cache", "head_dim_v", "shared_prefix_len", "cu_group_seqs", "max_group_seqs", "kv", "cache_seqlens", "block_table", "softmax_scale", "causal",
          "num_splits", "return_softmax_lse", "cascade"]
  params = inspect.signature(ffpa_attn_amd.ffpa_attn_with_kvcache_mla_cascade).parameters
  assert list(params) == want
  fp8 = inspect.signature(ffpa_attn_amd.ffpa_attn_with_kvcache_mla_cascade_fp8).parameters
  assert sorted(fp8) == sorted(want + ["kv_scale"]) and fp8["kv_scale"].default == 1.0
  for sig in (params, fp8):
    for name in list(sig)[3:]:
      assert sig[name].kind is inspect.Parameter.KEYWORD_ONLY, name
    assert sig["cascade"].default is None and sig["cu_group_seqs"].default is None and sig["max_group_seqs"].default is None
  assert list(inspect.signature(mla_cascade_rule).parameters) == ["batch", "seqlen_q", "heads_q", "heads_kv", "shared_prefix_len", "num_groups"]
  doc = ffpa_attn_amd.ffpa_attn_with_kvcache_mla_cascade.__doc__
  for phrase in ("UNCHECKED CONTRACT", "caller's race", "FIRST sequence", "device tensor", "max_group_seqs", "contiguous"):
    assert phrase in doc, phrase


# ---- the fakes and the routes on meta tensors
def test_the_plan_op_has_a_fake():
  outs = torch.ops.ffpa_attn._mla_cascade_plan_hip(_i32(6), _i32(6, 5), _i32(4), _i32(3), 0, 64, 2, 1, 320)
  assert [tuple(t.shape) for t in outs] == [(4,), (3,), (3, 5), (6, 5), (6,)]
  assert all(t.dtype == torch.int32 and t.device.type == "meta" for t in outs)
  outs = torch.ops.ffpa_attn._mla_cascade_plan_hip(_i32(6), _i32(6, 5), None, None, 128, 128, 1, 0, 640)
  assert [tuple(t.shape) for t in outs] == [(2,), (1,), (1, 5), (6, 5), (6,)]
  for args, exc in (((_i32(6), _i32(5, 5), None, None, 0, 64, 1, 0, 320), ValueError), ((_i32(6), _i32(6, 5), _i32(4), _i32(2), 0, 64, 1, 0, 320), ValueError),
                    ((_i32(6), _i32(6, 5), None, None, -1, 64, 1, 0, 320), ValueError), ((_i32(6), _i32(6, 5), None, None, 0, 96, 1, 0, 320), ValueError),
                    ((_i32(6), _i32(6, 5), None, None, 0, 64, 0, 0, 320), ValueError), ((_i32(6), _i32(6, 5), None, None, 0, 64, 1, 0, 321), ValueError),
                    ((_meta(6, dtype=torch.int64), _i32(6, 5), None, None, 0, 64, 1, 0, 320), TypeError)):
    with pytest.raises(exc):
      torch.ops.ffpa_attn._mla_cascade_plan_hip(*args)
  with pytest.raises(NotImplementedError):  # (no CPU kernel)
    hip.mla_cascade_plan(torch.zeros(2, dtype=torch.int32), torch.zeros(2, 3, dtype=torch.int32), None, None, 64, 64, 1, False, 192)


@pytest.mark.parametrize("name", CALLS)
@pytest.mark.parametrize("mode", [None, True, False])
@pytest.mark.parametrize("grouped", [False, True])
def test_shapes_on_meta(name, mode, grouped):
  """Every route end to end on meta tensors (every launch is a registered op with a fake): the append, the plan, both passes and the merge."""
  kw = dict(q=_meta(6, 3, 16, 576), kv=_meta(6, 3, 1, 576), causal=True, return_softmax_lse=True, cascade=mode)
  if grouped:
    kw.update(cu_group_seqs=_i32(4), shared_prefix_len=_i32(3), max_group_seqs=3)
  out, lse = _call(name, **kw)
  assert out.shape == (6, 3, 16, 512) and out.dtype == torch.bfloat16 and lse.shape == (6, 16, 3) and lse.dtype == torch.float32
  out = _call(name, q=_meta(6, 1, 128, 576, dtype=torch.float16), kv_cache=_meta(40, 128, 1, 576, dtype=torch.float8_e4m3fn if name.endswith("_fp8") else torch.float16),
              shared_prefix_len=0, cascade=mode)
  assert out.shape == (6, 1, 128, 512) and out.dtype == torch.float16
  for q in (_meta(0, 1, 16, 576), _meta(6, 0, 16, 576)):  # (no query token: the plain call's empty results)
    out, lse = _call(name, q=q, cache_seqlens=_i32(q.size(0)), block_table=_i32(q.size(0), 5), return_softmax_lse=True, cascade=mode)
    assert out.shape == (*q.shape[:3], 512) and lse.shape == (q.size(0), 16, q.size(1))


def test_cascade_none_asks_the_rule_for_a_host_int_and_takes_the_cascade_for_a_tensor(monkeypatch):
  from ffpa_attn_amd import kvcache

  asked, planned = [], []
  monkeypatch.setattr(kvcache, "mla_cascade_rule", lambda *a: asked.append(a) or False)
  real = torch.ops.ffpa_attn._mla_cascade_plan_hip

  class Spy(torch.utils._python_dispatch.TorchDispatchMode):
    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
      if func is real.default:
        planned.append(1)
      return func(*args, **(kwargs or {}))

  with Spy():
    _call(CALLS[0], shared_prefix_len=128, cu_group_seqs=_i32(4))
    assert asked == [(6, 1, 16, 1, 128, 3)] and not planned
    _call(CALLS[0], shared_prefix_len=_i32(3), cu_group_seqs=_i32(4))
    assert len(asked) == 1 and planned == [1]
    _call(CALLS[0], shared_prefix_len=_i32(3), cu_group_seqs=_i32(4), cascade=False)
    assert planned == [1]


def test_the_rule_table():
  # never for a batch without two sequences in some group, without a shared prefix, a token or a head
  for args in ((1, 1, 16, 1, 32768), (64, 1, 16, 1, 0), (64, 0, 16, 1, 32768), (8, 1, 16, 1, 1 << 20, 8), (64, 1, 16, 0, 32768), (64, 1, 16, 1, 32768, 0)):
    assert mla_cascade_rule(*args) is False, args
  # (B, Sq, Hq, Hkv, P, G) -> taken: 16 query heads on one latent head, one token, B x P >= 2^20 sequence-keys, 4 or more sequences per group
  table = [
    ((64, 1, 16, 1, 32768), True),
    ((64, 1, 16, 1, 32768, 8), True),
    ((64, 1, 16, 1, 32768, 16), True),    # groups of 4
    ((64, 1, 16, 1, 32768, 32), False),   # groups of 2: not measured
    ((64, 1, 16, 1, 16384, 8), True),     # exactly 2^20
    ((64, 1, 16, 1, 16383, 8), False),
    ((64, 1, 16, 1, 8192, 8), False),     # 2^19: lost eagerly
    ((16, 1, 16, 1, 32768), False),       # 2^19
    ((128, 1, 16, 1, 8192, 16), True),
    ((64, 4, 16, 1, 32768), False),       # 4 tokens: the tiles are full, measured as a loss
    ((64, 1, 128, 1, 32768), False),      # Hq 128: too narrow a win
    ((64, 1, 32, 2, 32768), False),       # two latent heads: not measured
    ((64, 1, 8, 1, 32768), False),        # 8 query heads: not measured
    ((64, 2, 8, 1, 32768), False),        # 16 rows of two tokens: not measured
  ]
  for args, taken in table:
    assert mla_cascade_rule(*args) is taken, args


def _measured_rows(name):
  with open(os.path.join(ROOT, "profiles", name)) as f:
    return json.load(f)["rows"]


def test_the_rule_never_takes_a_measured_loss_and_holds_off_its_grid():
  """Every shape of the committed A/B (tools/gpu_mla_cascade_ab.py on MI355X): where the rule takes the cascade, the cascade was faster, replayed from a graph
  and launched eagerly — on the grid it was fitted to and on the check rows off it."""
  for name, least_rows, least_taken in (("r26_mla_cascade.json", 70, 4), ("r26_mla_cascade_check.json", 15, 5)):
    rows = _measured_rows(name)
    assert len(rows) >= least_rows
    taken = 0
    for r in rows:
      rule = mla_cascade_rule(r["B"], r["Sq"], r["Hq"], r["Hkv"], r["P"], r["G"])
      assert rule is r["rule"], r
      if rule:
        taken += 1
        assert r["us"]["cascade"] < r["us"]["plain"] and r["us"]["cascade eager"] < r["us"]["plain eager"], r
    assert taken >= least_taken, name


# ---- the torch restatement of the plan, on cases worked by hand
def _table(B, W):
  return (torch.arange(B * W, dtype=torch.int32).view(B, W) * 3 + 7) % 101


def _lists(outs):
  return [t.tolist() for t in outs]


def test_ref_rounds_down_and_cuts_back_to_the_shortest_sequence():
  t = _table(3, 5)
  lens = torch.tensor([300, 200, 260], dtype=torch.int32)
  # stated 200 with pages of 64: rounded down to 192 = 3 pages
  cu, pl, pt, st, sl = ref_plan(lens, t, None, 200, 64, 1, False, 320)
  assert cu.tolist() == [0, 3] and pl.tolist() == [192] and sl.tolist() == [108, 8, 68]
  assert pt.tolist() == [t[0].tolist()]
  for b in range(3):
    r = t[b].tolist()
    assert st[b].tolist() == [r[3], r[4], r[4], r[4], r[4]]
  # stated 320 exceeds the shortest sequence (200): cut back to 200, then rounded down to 192; with pages of 128 to 128
  assert ref_plan(lens, t, None, 320, 64, 1, False, 320)[1].tolist() == [192]
  assert ref_plan(lens, t[:, :3], None, 320, 128, 1, False, 384)[1].tolist() == [128]
  # a page multiple every sequence holds stays
  assert ref_plan(lens, t, None, 128, 64, 1, False, 320)[1].tolist() == [128]
  assert all(x.dtype == torch.int32 for x in (cu, pl, pt, st, sl))


def test_ref_causal_leaves_the_first_token_its_keys():
  t = _table(2, 4)
  lens = torch.tensor([130, 200], dtype=torch.int32)
  # Sq 4 causal: the first query token of sequence 0 sees 130 - 3 = 127 keys: one page, not two
  assert ref_plan(lens, t, None, 128, 64, 4, True, 256)[1].tolist() == [64]
  assert ref_plan(lens, t, None, 128, 64, 4, False, 256)[1].tolist() == [128]
  assert ref_plan(lens, t, None, 128, 64, 3, True, 256)[1].tolist() == [128]  # (130 - 2 = 128)
  cu, pl, pt, st, sl = ref_plan(lens, t, None, 128, 64, 4, True, 256)
  assert cu.tolist() == [0, 8] and sl.tolist() == [66, 136]
  # shorter than the tokens: nothing is shared
  assert ref_plan(torch.tensor([2, 200], dtype=torch.int32), t, None, 128, 64, 4, True, 256)[1].tolist() == [0]


def test_ref_groups_with_an_empty_one_and_lengths_outside_the_cache():
  t = _table(5, 4)
  lens = torch.tensor([256, 300, -5, 70, 200], dtype=torch.int32)  # (300 > capacity 256: clamped; -5: 0)
  cu_g = torch.tensor([0, 2, 2, 3, 5], dtype=torch.int32)
  stated = torch.tensor([1000, 64, 64, 100], dtype=torch.int32)
  cu, pl, pt, st, sl = ref_plan(lens, t, cu_g, stated, 64, 2, False, 256)
  assert cu.tolist() == [0, 4, 4, 6, 10]
  assert pl.tolist() == [256, 0, 0, 64]  # (group 0: both hold the capacity; 1: empty; 2: a negative length holds nothing; 3: min(100, 70) -> 64)
  assert sl.tolist() == [0, 0, 0, 6, 136]
  assert pt[0].tolist() == t[0].tolist() and pt[2].tolist() == t[2].tolist() and pt[3].tolist() == t[3].tolist()
  assert pt[1].tolist() in [r.tolist() for r in t]
  # a shift past the table's width: every column of the suffix row is the last page's
  assert st[0].tolist() == [int(t[0, 3])] * 4 and st[1].tolist() == [int(t[1, 3])] * 4
  assert st[2].tolist() == t[2].tolist() and st[3].tolist() == t[3].tolist()[1:] + [int(t[3, 3])]
  # the same groups with one host int
  assert ref_plan(lens, t, cu_g, 128, 64, 2, False, 256)[1].tolist() == [128, 0, 0, 64]
  # an empty group behind the last sequence
  cu, pl, pt, st, sl = ref_plan(lens, t, torch.tensor([0, 5, 5], dtype=torch.int32), 64, 64, 1, False, 256)
  assert pl.tolist() == [0, 0] and cu.tolist() == [0, 5, 5] and pt[1].tolist() == t[4].tolist()
