"""In-tree build of the gfx950 C-ABI library (``libffpa_attn_hip.so``).

The reference drives nvcc through setup.py/env.py and generates one TU per
(dtype, acc, headdim, stage) (``env.py:455-521``, ``setup.py:112-145``).  Here the
library has no torch / pybind dependency, so the build is plain ``hipcc``: one
object per head dim (compiled in parallel) + the C-ABI object, linked into a
shared library that stays next to the sources (it travels to the GPU box with the
repo snapshot; a JIT cache would not).

Usage:  python -m ffpa_attn_amd.build [--force] [--jobs N] [--no-test-lib]
"""

from __future__ import annotations

import argparse
import collections
import os
import re
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
REPO = os.path.dirname(HERE)
INCLUDE = os.path.join(REPO, "include")
OBJ_DIR = os.path.join(CSRC, "build")
LIB_NAME = "libffpa_attn_hip.so"
LIB_PATH = os.path.join(HERE, LIB_NAME)
TEST_LIB_PATH = os.path.join(HERE, "libffpa_attn_hip_test.so")

HEAD_DIMS = [64 * i for i in range(1, 17)]
# head dims whose test-only "safe path" twin kernel (register staging + scalar V gather, used to bisect
# LDS-DMA / transpose-read problems on hardware) is built into libffpa_attn_hip_test.so — never into the product library.
SAFE_HEAD_DIMS = {64, 128, 320, 512, 640, 1024}
# head dims the packed-sequence kernel is built for (FFPA_FOR_EACH_VARLEN_HEAD_DIM, csrc/ffpa_launch.h): the 16x16x32 build's
VARLEN_HEAD_DIMS = [d for d in HEAD_DIMS if d >= 128]
# (head dim, value width) pairs the MLA latent-cache kernel is built for (FFPA_FOR_EACH_MLA_BUILD, csrc/ffpa_mla.h)
MLA_BUILDS = [(576, 512)]
# the variants of that kernel, by the stem of their row in FFPA_FOR_EACH_MLA_VARIANT (csrc/ffpa_mla.h), in its order: the link order
MLA_VARIANTS = ["mla", "mla_sparse", "mla_tree", "mla_fp8", "mla_sparse_fp8", "mla_tree_fp8", "mla_sparse_ds"]

ARCH = "gfx950"
CXXFLAGS = [
  f"--offload-arch={ARCH}",
  "-O3",
  "-std=c++17",
  "-fPIC",
  "-mcode-object-version=5",
  f"-I{INCLUDE}",
  f"-I{CSRC}",
]

# One row per translation unit: source under csrc/, object under csrc/build/, its own -D defines, the directory its -save-temps output lands in (None: not kept;
# the attention ISA rules read every *.s of temps_d<D>, so the packed and paged kernels' assembly lands next to the dense TU's), the head dim it instantiates,
# and which library links it.  The rows are in link order.
Unit = collections.namedtuple("Unit", "src obj defs temps dim product test")


def _units() -> list[Unit]:
  units = []
  for d in HEAD_DIMS:
    inst = [f"-DFFPA_INST_D={d}"]
    safe = d in SAFE_HEAD_DIMS  # (the test library links the twin that carries the SAFE kernels instead)
    units.append(Unit("ffpa_fwd_inst.hip", f"ffpa_fwd_d{d}.o", inst, f"temps_d{d}", d, True, not safe))
    if safe:
      units.append(Unit("ffpa_fwd_inst.hip", f"ffpa_fwd_d{d}_test.o", inst + ["-DFFPA_INST_SAFE=1"], None, d, False, True))
  # the packed-sequence kernel and its paged-KV twin: a TU of their own per head dim of the 16x16x32 build
  for kind in ("varlen", "paged"):
    units += [Unit(f"ffpa_{kind}_inst.hip", f"ffpa_{kind}_d{d}.o", [f"-DFFPA_INST_D={d}"], f"temps_d{d}", d, True, True) for d in VARLEN_HEAD_DIMS]
  # the MLA latent-cache kernels: one TU per variant (MLA_VARIANTS; ffpa_mla_inst.hip and ffpa_mla_fp8_inst.hip carry the appends too) and (head dim, value width)
  # pair of MLA_BUILDS; the assembly lands next to the head dim's other kernels, where the ISA rules read it.  Behind them the small kernel that writes 656-byte
  # rows by slot (no inline asm: its assembly lands where the attention ISA rules do not read)
  for stem in MLA_VARIANTS:
    units += [Unit(f"ffpa_{stem}_inst.hip", f"ffpa_{stem}_d{d}.o", [f"-DFFPA_INST_D={d}"], f"temps_d{d}", d, True, True) for d, _ in MLA_BUILDS]
  units.append(Unit("ffpa_mla_ds_store.hip", "ffpa_mla_ds_store.o", [], "temps_mla_store", None, True, True))
  # the launch that makes the sparse calls' inputs — top-k selection over an indexer's scores and the block-table translation — one small kernel (no inline asm)
  units.append(Unit("ffpa_mla_sparse_topk.hip", "ffpa_mla_sparse_topk.o", [], "temps_mla_sparse_topk", None, True, True))
  # the KV-cache append + rotary launch (every dtype / rotary form) and the merge of two attention states (the cascade's last launch): one small TU each, no
  # inline asm — their assembly lands in directories the attention ISA rules do not read
  units.append(Unit("ffpa_kvcache_append.hip", "ffpa_kvcache_append.o", [], "temps_append", None, True, True))
  units.append(Unit("ffpa_merge_states.hip", "ffpa_merge_states.o", [], "temps_merge", None, True, True))
  # the append for a ragged step (token rows packed by cu_seqlens_q, per-token rotary positions): shares ffpa_kvcache_append_rows.h with the [B, S] append
  units.append(Unit("ffpa_kvcache_append_varlen.hip", "ffpa_kvcache_append_varlen.o", [], "temps_append_varlen", None, True, True))
  # the plan launch of a shared-prefix (cascade) step over the MLA latent cache: group boundaries, effective prefix lengths and the two passes' tables in one
  # small kernel (no inline asm)
  units.append(Unit("ffpa_mla_cascade_plan.hip", "ffpa_mla_cascade_plan.o", [], "temps_mla_cascade_plan", None, True, True))
  units.append(Unit("ffpa_capi.hip", "ffpa_capi.o", [], None, None, True, False))
  units.append(Unit("ffpa_capi.hip", "ffpa_capi_test.o", ["-DFFPA_INST_SAFE=1"], None, None, False, True))
  return units


UNITS = _units()
# the product define: the kernel headers then refuse any developer switch that is not at its shipped default
PRODUCT_DEFS = ["-DFFPA_PRODUCT_BUILD=1"]


def _compile_cmd(hipcc: str, u: Unit, defs: list[str], obj: str, save_temps: bool = False) -> list[str]:
  return [hipcc, *CXXFLAGS, *defs, *(["-save-temps"] if save_temps and u.temps else []), *u.defs, "-c", os.path.join(CSRC, u.src), "-o", obj]


def _link(hipcc: str, lib: str, objs: list[str]) -> None:
  _run([hipcc, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", lib, *objs, "-Wl,-rpath,/opt/rocm/lib"])


def _hipcc() -> str:
  for cand in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
    if cand and os.path.exists(cand):
      return cand
  raise RuntimeError("hipcc not found: the HIP toolchain is required to build ffpa_attn_amd")


def _sources_mtime() -> float:
  paths = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".h", ".hip", ".inc"))]
  paths.append(os.path.join(INCLUDE, "ffpa_attn.h"))
  paths.append(os.path.abspath(__file__))
  return max(os.path.getmtime(p) for p in paths)


def _run(cmd: list[str], cwd: str | None = None) -> None:
  proc = subprocess.run(cmd, capture_output=True, text=True, cwd=cwd)
  if proc.returncode != 0:
    raise RuntimeError("command failed: " + " ".join(cmd) + "\n" + proc.stdout + proc.stderr)


def _check_isa(verbose: bool) -> None:
  """The S^T MFMAs and the LDS-DMA are inline asm (no compiler hazard padding, M0 written behind the compiler's
  back): prove on the ISA just generated that no VALU write lands in an MFMA operand's hazard window and that
  nothing outside the DMA asm touches M0 (tools/check_mfma_hazards.py).  A violation fails the build."""
  import importlib.util

  path = os.path.join(REPO, "tools", "check_mfma_hazards.py")
  if not os.path.exists(path):  # an installed copy without the developer tools
    return
  spec = importlib.util.spec_from_file_location("check_mfma_hazards", path)
  chk = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(chk)
  import contextlib, io

  old_argv, sys.argv = sys.argv, ["check_mfma_hazards"]
  buf = io.StringIO()
  try:
    with contextlib.redirect_stdout(buf):
      rc = chk.main()
  finally:
    sys.argv = old_argv
  if verbose or rc != 0:
    print(buf.getvalue(), end="", flush=True)
  if rc != 0:
    raise RuntimeError("ISA check failed: an inline-asm MFMA operand is written inside its hazard window, or M0 is written outside the DMA asm")


def _prune_temps() -> None:
  """-save-temps leaves ~20 MB per TU (bitcode, preprocessed source, host assembly ...) and the whole tree travels to the GPU box with every
  snapshot.  What the ISA rules (tools/check_mfma_hazards.py, tools/isa_stats.py, tests/test_isa_rules.py) read is the device assembly alone: it
  stays, gzip-compressed (10 : 1); everything else goes.  354 MB -> ~6 MB."""
  import glob
  import gzip

  for tdir in glob.glob(os.path.join(OBJ_DIR, "temps_*")):
    for path in glob.glob(os.path.join(tdir, "*")):
      if path.endswith("gfx950.s"):
        with open(path, "rb") as src, gzip.open(path + ".gz", "wb", compresslevel=6) as dst:
          shutil.copyfileobj(src, dst)
      elif path.endswith("gfx950.s.gz") and not os.path.exists(path[:-3]):
        continue  # (the assembly of a TU this run did not recompile)
      if os.path.isdir(path):
        shutil.rmtree(path, ignore_errors=True)
      else:
        os.remove(path)


def clean_dev(objects: bool = True) -> None:
  """Remove what only a development session needs and the round-end snapshot should not carry: variant libraries (build_variant) and their objects — and, with
  ``objects``, the object files of the main build once both libraries are linked and fresh (20 MB; ``build()`` is gated on the libraries' mtime, and
  ``build_variant --dims`` rebuilds the objects it finds missing)."""
  import glob

  shutil.rmtree(os.path.join(HERE, "variants"), ignore_errors=True)
  for d in glob.glob(os.path.join(OBJ_DIR, "var_*")):
    shutil.rmtree(d, ignore_errors=True)
  _prune_temps()
  if objects and os.path.exists(LIB_PATH) and os.path.exists(TEST_LIB_PATH):
    newest = _sources_mtime()
    if os.path.getmtime(LIB_PATH) >= newest and os.path.getmtime(TEST_LIB_PATH) >= newest:
      for o in glob.glob(os.path.join(OBJ_DIR, "*.o")):
        os.remove(o)


def build(force: bool = False, jobs: int | None = None, save_temps: bool = True, verbose: bool = True, test_lib: bool = True) -> str:
  """Compile every kernel for gfx950, link ``libffpa_attn_hip.so`` (product kernels only) and — with ``test_lib`` —
  ``libffpa_attn_hip_test.so`` (the same library plus the register-staged SAFE twins behind FFPA_FLAG_DEBUG_SAFE_PATH,
  used by the GPU tests to bisect the LDS-DMA / transpose-read data path); returns the product library's path.
  The generated ISA is kept (``-save-temps``) and checked for the hazards the inline asm hides from the compiler."""
  newest = _sources_mtime()
  have = os.path.exists(LIB_PATH) and os.path.getmtime(LIB_PATH) >= newest
  have_test = not test_lib or (os.path.exists(TEST_LIB_PATH) and os.path.getmtime(TEST_LIB_PATH) >= newest)
  if not force and have and have_test:
    return LIB_PATH
  hipcc = _hipcc()
  os.makedirs(OBJ_DIR, exist_ok=True)
  jobs = jobs or max(1, (os.cpu_count() or 4))
  tasks: list[tuple[str, list[str], str | None]] = []
  units = [u for u in UNITS if u.product or test_lib]
  for u in units:
    obj = os.path.join(OBJ_DIR, u.obj)
    if force or not os.path.exists(obj) or os.path.getmtime(obj) < newest:
      tmp = os.path.join(OBJ_DIR, u.temps) if save_temps and u.temps else None  # temps land in the compile's cwd (one dir per TU)
      if tmp:
        os.makedirs(tmp, exist_ok=True)
      tasks.append((obj, _compile_cmd(hipcc, u, PRODUCT_DEFS, obj, save_temps), tmp))
  if verbose:
    print(f"[ffpa_attn_amd.build] compiling {len(tasks)} objects for {ARCH} with {jobs} jobs", flush=True)
  # longest jobs first (head dims >= 320 carry the 16x16x32 builds as well: 2 - 3 x the compile time of the small ones)
  def cost(t):
    m = re.search(r"ffpa_fwd_d(\d+)", t[0])
    return -(int(m.group(1)) + (2048 if m and int(m.group(1)) >= 320 else 0)) if m else 0

  tasks.sort(key=cost)
  with ThreadPoolExecutor(max_workers=jobs) as pool:
    list(pool.map(lambda t: _run(t[1], cwd=t[2]), tasks))
  if save_temps:
    _check_isa(verbose)
    _prune_temps()
  _link(hipcc, LIB_PATH, [os.path.join(OBJ_DIR, u.obj) for u in units if u.product])
  if test_lib:
    _link(hipcc, TEST_LIB_PATH, [os.path.join(OBJ_DIR, u.obj) for u in units if u.test])
  if verbose:
    print(f"[ffpa_attn_amd.build] linked {LIB_PATH}" + (f" and {TEST_LIB_PATH}" if test_lib else ""), flush=True)
  return LIB_PATH


def build_variant(tag: str, defs: list[str], jobs: int | None = None, head_dims: list[int] | None = None) -> str:
  """Developer tool: build ``variants/libffpa_attn_hip_<tag>.so`` with extra ``-D`` tunables (see the
  FFPA_* macros at the top of csrc/ffpa_fwd_kernel.h) for A/B timing with tools/gpu_ab.py.  With
  ``head_dims`` only those head dims are recompiled with the tunables; the rest of the C-ABI table
  links the objects of the main build (which must exist), so a variant costs seconds."""
  hipcc = _hipcc()
  odir = os.path.join(OBJ_DIR, f"var_{tag}")
  os.makedirs(odir, exist_ok=True)
  vdir = os.path.join(HERE, "variants")
  os.makedirs(vdir, exist_ok=True)
  lib = os.path.join(vdir, f"libffpa_attn_hip_{tag}.so")
  newest = _sources_mtime()
  stamp = os.path.join(odir, "defs.txt")
  key = " ".join(defs) + " | " + ",".join(str(d) for d in (head_dims or HEAD_DIMS))
  same_defs = os.path.exists(stamp) and open(stamp).read() == key
  if same_defs and os.path.exists(lib) and os.path.getmtime(lib) >= newest:
    return lib
  # what the variant compiles itself: the dense TUs of its head dims and the C-ABI object (the plan must see the same tunables as the kernels); everything else —
  # the untouched head dims, the packed-sequence kernels and their paged twins, the KV-cache append, the state merge — is the main build's object, never a
  # variant's (a round-end clean_dev() may have removed them: rebuilt then)
  def own(u: Unit) -> bool:
    return u.src == "ffpa_capi.hip" or (u.src == "ffpa_fwd_inst.hip" and (not head_dims or u.dim in head_dims))

  units = [u for u in UNITS if u.product]
  missing = any(not own(u) and not os.path.exists(os.path.join(OBJ_DIR, u.obj)) for u in units)
  if head_dims or missing:
    build(force=missing, verbose=False)
  objs = [os.path.join(odir if own(u) else OBJ_DIR, u.obj) for u in units]
  tasks = [_compile_cmd(hipcc, u, defs, os.path.join(odir, u.obj)) for u in units if own(u)]
  with ThreadPoolExecutor(max_workers=jobs or (os.cpu_count() or 4)) as pool:
    list(pool.map(_run, tasks))
  _link(hipcc, lib, objs)
  with open(stamp, "w") as f:
    f.write(key)
  return lib


def main() -> None:
  ap = argparse.ArgumentParser(description=__doc__)
  ap.add_argument("--force", action="store_true")
  ap.add_argument("--jobs", type=int, default=None)
  ap.add_argument("--save-temps", action="store_true", help="(default now: the generated ISA is always kept and checked)")
  ap.add_argument("--no-test-lib", action="store_true", help="skip libffpa_attn_hip_test.so (the SAFE twin kernels the GPU tests use)")
  ap.add_argument("--variant", nargs="+", metavar=("TAG", "DEF"), help="build variants/libffpa_attn_hip_TAG.so with -D defs")
  ap.add_argument("--dims", type=lambda s: [int(x) for x in s.split(",")], default=None, help="variant: only recompile these head dims")
  ap.add_argument("--clean-dev", action="store_true", help="remove variants/ and their objects, prune the ISA temps (what a round-end snapshot should not carry)")
  args = ap.parse_args()
  if args.clean_dev:
    clean_dev()
    return
  if args.variant:
    print(build_variant(args.variant[0], [d if d.startswith("-D") else "-D" + d for d in args.variant[1:]], jobs=args.jobs, head_dims=args.dims))
    return
  print(build(force=args.force, jobs=args.jobs, test_lib=not args.no_test_lib))


if __name__ == "__main__":
  sys.exit(main())
