"""bench.py pieces that need no GPU: the HBM-traffic figure is quoted only from a profile of the very library that runs (round-3 review:
the line read a committed file with no check that it described the running binary)."""

import importlib.util
import json
import os

from conftest import ROOT


def _bench():
  spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  return mod


def test_traffic_is_only_quoted_from_a_profile_of_the_running_library(tmp_path, monkeypatch):
  bench = _bench()
  prof = tmp_path / "profiles"
  prof.mkdir()
  doc = {"provenance": {"lib_sha16": "aaaabbbbccccdddd"}, "derived": {"hbm_read_bytes_corrected_x2": 1000.0, "hbm_write_bytes": 24.0}}
  (prof / "r04_bench_cfg2_pmc.json").write_text(json.dumps(doc))
  monkeypatch.setattr(bench, "ROOT", str(tmp_path))
  assert bench.measured_traffic("cfg2", "aaaabbbbccccdddd") == (1024, os.path.join("profiles", "r04_bench_cfg2_pmc.json"), False)
  traffic, src, stale = bench.measured_traffic("cfg2", "0000000000000000")
  assert traffic is None and stale is True and src.endswith("r04_bench_cfg2_pmc.json")  # another binary's profile: named, not quoted
  assert bench.measured_traffic("cfg2", None)[0] is None                                # the running library's sha is unknown: not quoted either
  assert bench.measured_traffic("cfg3", "aaaabbbbccccdddd") == (None, None, False)       # no profile committed


def test_committed_r04_profiles_name_their_binary():
  """Every committed round-4 PMC summary carries the library sha / git head / clock it was taken with."""
  import glob

  files = glob.glob(os.path.join(ROOT, "profiles", "r04_bench_*_pmc*.json"))
  assert files
  for f in files:
    prov = json.load(open(f)).get("provenance", {})
    assert len(prov.get("lib_sha16", "")) == 16 and prov.get("git_head") and prov.get("bench_kernel"), f


def test_dump_outputs_writes_float32_whole_or_a_fixed_sample(tmp_path):
  """`--dump-outputs`: a small output whole (shape kept), a large one as the same seeded sample of positions every time, float32, <= 16 MB per array."""
  import numpy as np
  import torch

  bench = _bench()
  small = torch.randn(2, 3, 5, 7, dtype=torch.bfloat16)
  lse = torch.randn(2, 3, 5, dtype=torch.float32)
  got = bench.dump_outputs(str(tmp_path / "a"), (small, lse))
  assert set(got["arrays"]) == {"out", "lse"} and got["arrays"]["out"]["saved"] == "whole"
  o = np.load(tmp_path / "a" / "out.npy")
  assert o.dtype == np.float32 and o.shape == (2, 3, 5, 7) and np.array_equal(o, small.float().numpy())
  assert np.array_equal(np.load(tmp_path / "a" / "lse.npy"), lse.numpy())

  big = torch.arange(bench.DUMP_WHOLE_MAX * 3, dtype=torch.float32).reshape(3, -1)
  for d in ("b", "c"):
    bench.dump_outputs(str(tmp_path / d), big)
  b, c = np.load(tmp_path / "b" / "out.npy"), np.load(tmp_path / "c" / "out.npy")
  assert b.dtype == np.float32 and b.nbytes <= 16 << 20 and np.array_equal(b, c)
  assert b.size > bench.DUMP_WHOLE_MAX // 2 and (np.diff(b) > 0).all() and b.max() < big.numel()  # distinct positions in index order, the values at them
  assert not (tmp_path / "b" / "lse.npy").exists()
