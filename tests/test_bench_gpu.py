"""bench.py on one GPU: a plain run's one JSON line holds the contract's keys and nothing measured after the timed region; with --full the line
also has the roofline and CPU-baseline objects, what the device said about itself, and the steady-state leg.  No throughput is asserted — only
that the line is whole and self-consistent."""

import json
import os
import subprocess
import sys

import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu


def _bench(*flags):
  env = dict(os.environ)
  for k_ in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
    env.pop(k_, None)
  out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *flags], capture_output=True, text=True, timeout=600, env=env)
  assert out.returncode == 0, out.stderr[-2000:]
  lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
  assert len(lines) == 1, out.stdout[-2000:]
  return json.loads(lines[0])


FULL_ONLY = ("roofline", "steady_state", "build", "plan", "ref_protocol", "cpu_baseline", "max_abs_err_vs_sdpa", "sdpa_gpu_ms", "decode_step", "graph_replay",
             "other_launches", "per_sequence_loop", "with_gather")


@pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")
def test_plain_run_prints_the_headline_and_nothing_measured_after_it():
  """Without --full a run sets up, warms up, times the steps and prints the line: the contract's keys, and no leg that runs after the timed region."""
  for workload, steps, warmup in (("cfg2", 3, 1), ("varlen", 3, 1), ("varlen_decode", 4, 2)):
    line = _bench("--gpus", "1", "--workload", workload, "--steps", str(steps), "--warmup", str(warmup))
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config", "device"):
      assert key in line, (workload, key)
    assert not [k_ for k_ in FULL_ONLY if k_ in line], (workload, sorted(line))
    assert line["steps"] == steps and line["warmup"] == warmup and line["unit"] == "TFLOPS" and line["higher_is_better"] is True and line["dtype"] == "bf16"
    assert line["value"] > 0 and line["ms_per_step"] > 0
  assert line["device"]["cus"] == torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")
def test_bench_line_of_a_short_workload_is_whole():
  line = _bench("--gpus", "1", "--workload", "cross", "--steps", "4", "--warmup", "2", "--full", "--no-sdpa")
  for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
              "roofline", "cpu_baseline", "device", "steady_state", "build", "plan"):
    assert key in line, key
  assert line["n_gpus"] == 1 and line["steps"] == 4 and line["warmup"] == 2 and line["dtype"] == "bf16" and line["vs_baseline"] is None
  assert "model" not in line["config"] and line["config"]["workload"].startswith("cross")
  roof = line["roofline"]
  assert roof["bound"] == "mfma" and roof["unit"] == "TFLOP/s" and roof["peak"] == 2500.0 and "traffic" in roof
  # round 6: the HBM traffic of the dominant kernel is MEASURED in the run (two rocprofv3 PMC passes of the same command behind the timed region) — at least the
  # compulsory bytes, and nowhere near the operand stream the kernel re-reads from L2 (a counter in the wrong unit would be off by 1024 or more)
  if "traffic_live_failed" not in roof:
    assert roof["traffic_source"].startswith("measured in this run") and roof["traffic_stale"] is False
    assert 0.8 * roof["algorithmic_bytes_per_launch"] <= roof["traffic"] <= 20 * roof["algorithmic_bytes_per_launch"], roof
  else:
    assert isinstance(roof["traffic_live_failed"], str) and roof["traffic_live_failed"]
  assert abs(roof["frac"] - roof["achieved"] / roof["peak"]) < 1e-3 and 0.0 < roof["frac"] < 1.0
  assert roof["kernel"].startswith("ffpa_fwd_m16_kernel<bf16, 512")
  # the step cannot be shorter than its kernel, and the value follows from the step time
  assert roof["kernel_ms_avg"] <= line["ms_per_step"] * 1.02
  assert abs(line["value"] - roof["flops_per_launch"] / line["ms_per_step"] / 1e9) / line["value"] < 0.01
  cpu = line["cpu_baseline"]
  assert cpu["kind"] in ("reference", "port") and cpu["value"] > 0 and cpu["cores"] >= 1 and cpu["sample"]
  assert line["device"]["cus"] == torch.cuda.get_device_properties(0).multi_processor_count
  steady = line["steady_state"]
  assert steady["launches"] >= 20 and steady["after_launches"] >= 20 and steady["ms_per_step"] > 0
  assert abs(steady["tflops"] - roof["flops_per_launch"] / steady["ms_per_step"] / 1e9) / steady["tflops"] < 0.01
  assert line["build"]["lib"].endswith("libffpa_attn_hip.so") and len(line["build"]["lib_sha16"]) == 16


@pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")
def test_decode_line_is_priced_against_hbm_and_carries_the_graph_replay_leg():
  """The decode workload's roofline is the HBM one; its step is launch-bound from Python, so the line also says what the same step does when it is
  captured into a HIP graph and replayed (one step per graph, and 32 — a token's layers)."""
  line = _bench("--gpus", "1", "--workload", "decode", "--steps", "10", "--warmup", "3", "--full", "--no-sdpa", "--no-cpu-baseline", "--no-live-traffic")
  roof = line["roofline"]
  assert roof["bound"] == "hbm" and roof["unit"] == "GB/s" and roof["peak"] == 8000.0 and 0.0 < roof["frac"] < 1.0
  assert roof["kernel"].startswith("ffpa_fwd_split_d_kernel<bf16, 512")
  g = line["graph_replay"]
  assert "error" not in g, g
  for key in ("steps_per_graph_1", "steps_per_graph_32"):
    leg = g[key]
    assert leg["ms_per_step"] > 0 and abs(leg["gbps"] - roof["bytes_per_launch"] / leg["ms_per_step"] / 1e6) / leg["gbps"] < 0.01 and 0.0 < leg["frac_of_hbm_peak"] < 1.0
  # no host work per step: a replayed step cannot be slower than the step launched from Python by more than timer noise
  assert g["steps_per_graph_32"]["ms_per_step"] <= line["ms_per_step"] * 1.10


@pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")
def test_packed_decode_line_is_priced_against_hbm_and_names_its_launch():
  """`--workload varlen_decode`: a packed decode batch (one token per sequence, ragged KV lengths, GQA) — the HBM roofline of one step, the launch the library
  picked (heads packed into tile rows, KV ranges split and merged, the non-temporal fetch) and the same call without each of them beside it."""
  line = _bench("--gpus", "1", "--workload", "varlen_decode", "--steps", "4", "--warmup", "2", "--full", "--no-live-traffic")
  for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config", "roofline",
              "device", "steady_state", "build", "plan", "other_launches", "per_sequence_loop"):
    assert key in line, key
  roof = line["roofline"]
  assert roof["bound"] == "hbm" and roof["unit"] == "GB/s" and roof["peak"] == 8000.0 and 0.05 < roof["frac"] < 1.0
  assert abs(roof["achieved"] - roof["algorithmic_bytes_per_launch"] / (roof["kernel_ms_avg"] * 1e-3) / 1e9) <= 0.01 * roof["achieved"]
  assert "packed into rows" in roof["kernel"] and line["plan"]["workgroups"] == 32 * 8 * line["plan"]["splits"]
  legs = line["other_launches"]
  assert legs["one_kv_range"]["splits"] == 1 and legs["one_workgroup_per_query_head"]["workgroups"] % (32 * 32) == 0 and ", NT>" not in legs["no_nt_hint"]["kernel"]
  assert line["per_sequence_loop"]["max_abs_diff_vs_packed"] < 4e-3 and line["max_abs_err_vs_sdpa"] < 1e-2


@pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")
def test_dump_outputs_are_the_timed_paths_result_and_repeat_run_to_run(tmp_path):
  """`--dump-outputs DIR`: the last timed step's O as float32 (a seeded sample: the cross workload's O has 16 Mi elements), identical in two runs of the same
  command, and the values SDPA gives at the same positions for the same seed-0 inputs; the packed decode call dumps its O and LSE whole."""
  import numpy as np

  flags = ("--gpus", "1", "--workload", "cross", "--steps", "3", "--warmup", "1", "--no-sdpa", "--no-cpu-baseline", "--no-live-traffic", "--no-steady", "--no-ref-protocol")
  runs = [_bench(*flags, "--dump-outputs", str(tmp_path / d)) for d in ("a", "b")]
  assert all(r["steps"] == 3 and r["ms_per_step"] > 0 for r in runs)
  desc = runs[0]["dump_outputs"]["arrays"]
  assert list(desc) == ["out"] and desc["out"]["shape"] == [1, 32, 1024, 512] and desc["out"]["saved"].startswith("sample")
  a, b = np.load(tmp_path / "a" / "out.npy"), np.load(tmp_path / "b" / "out.npy")
  assert a.dtype == np.float32 and np.array_equal(a, b)
  dev = torch.device("cuda:0")
  torch.manual_seed(0)
  q = torch.randn(1, 32, 1024, 512, dtype=torch.bfloat16, device=dev)
  k = torch.randn(1, 32, 8192, 512, dtype=torch.bfloat16, device=dev)
  v = torch.randn(1, 32, 8192, 512, dtype=torch.bfloat16, device=dev)
  ref = torch.nn.functional.scaled_dot_product_attention(q, k, v).float().reshape(-1).cpu().numpy()
  idx = np.unique(np.random.default_rng(0).integers(0, ref.size, size=1 << 22))  # (the bench's draw: DUMP_WHOLE_MAX integers)
  assert idx.size == a.size
  err = np.abs(a - ref[idx])
  assert (err <= 2.0 ** -7 * np.abs(ref[idx]) + 2e-3).all() and err.mean() < 0.05 * np.abs(ref[idx]).mean(), (err.max(), err.mean())

  line = _bench("--gpus", "1", "--workload", "varlen_decode", "--steps", "2", "--warmup", "1", "--no-sdpa", "--no-cpu-baseline", "--no-live-traffic", "--no-steady",
                "--dump-outputs", str(tmp_path / "c"))
  desc = line["dump_outputs"]["arrays"]
  assert desc["out"]["shape"] == [32, 32, 512] and desc["out"]["saved"] == "whole" and desc["lse"]["saved"] == "whole"
  o, lse = np.load(tmp_path / "c" / "out.npy"), np.load(tmp_path / "c" / "lse.npy")
  assert o.shape == (32, 32, 512) and np.isfinite(o).all() and np.isfinite(lse).all() and lse.dtype == np.float32
