"""Host cost of the C layer's latent planner, on the CPU: time per *_plan query of one accepted call of each of the seven latent forms, this tree's library
against a saved build of another commit.

    python tools/cpu_capi_plan_cost.py --parent PATH/libffpa_attn_hip.so [--blocks 60] [--calls 20000]

Three arms — parent, tree, parent again (the same file loaded a second time through a copy, so that it is a library of its own) — interleaved block by block in one
process, the order rotating from block to block; per arm and form the minimum, lower quartile and median over the blocks, in nanoseconds per query (the ctypes call included: it is the same in every
arm).  The yardstick for the tree is the distance between the two parent arms.  The calls are the default call of each form of
tests/golden/make_capi_varlen_calls.py (D = 576, dv = 512, 16 heads on one latent head, one token per sequence); no device is touched."""

import argparse
import ctypes
import importlib.util
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FORMS = ("mla", "mla_tree", "sparse", "mla_fp8", "mla_tree_fp8", "sparse_fp8", "sparse_ds")


def main():
  ap = argparse.ArgumentParser(description=__doc__)
  ap.add_argument("--parent", required=True)
  ap.add_argument("--blocks", type=int, default=60)
  ap.add_argument("--calls", type=int, default=20000)
  args = ap.parse_args()
  from ffpa_attn_amd import hip

  spec = importlib.util.spec_from_file_location("recorder", os.path.join(ROOT, "tests", "golden", "make_capi_varlen_calls.py"))
  rec = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(rec)
  with tempfile.TemporaryDirectory() as tmp:
    twin = shutil.copy(args.parent, os.path.join(tmp, "parent_again.so"))
    arms = [("parent", hip.load_library(args.parent)), ("tree", hip.load_library(hip.LIB_PATH)), ("parent again", hip.load_library(twin))]
    times = {(arm, form): [] for arm, _ in arms for form in FORMS}
    plan = (ctypes.c_int * 5)()
    calls = {}
    for form in FORMS:
      keep, argv = rec._structs(hip, {"form": form})
      calls[form] = (keep, argv)
      for arm, lib in arms:
        assert getattr(lib, rec.FORMS[form][0] + "_plan")(*argv, plan) == 0, (arm, form)
    for block in range(args.blocks):
      for form in FORMS:
        _, argv = calls[form]
        for arm, lib in arms[block % 3:] + arms[:block % 3]:  # (the place in the round costs a few ns of its own: every arm takes every place)
          fn = getattr(lib, rec.FORMS[form][0] + "_plan")
          t0 = time.perf_counter_ns()
          for _ in range(args.calls):
            fn(*argv, plan)
          times[(arm, form)].append((time.perf_counter_ns() - t0) / args.calls)
  print(f"ns per *_plan query: minimum / lower quartile / median over {args.blocks} blocks of {args.calls} calls")
  print("| form | " + " | ".join(arm for arm, _ in arms) + " |")
  print("|---|---|---|---|")
  for form in FORMS:
    cells = []
    for arm, _ in arms:
      t = sorted(times[(arm, form)])
      cells.append(f"{t[0]:.1f} / {statistics.quantiles(t, n=4)[0]:.1f} / {statistics.median(t):.1f}")
    print(f"| `{rec.FORMS[form][0]}_plan` | " + " | ".join(cells) + " |")


if __name__ == "__main__":
  main()
