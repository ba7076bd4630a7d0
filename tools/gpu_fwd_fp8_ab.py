#!/usr/bin/env python
"""A/B of the FP8 forward against the bf16 forward on the same tensors (MI355X): ``ffpa_attn_fp8_func`` (pre-pass + kernel), the attention kernel alone
(``ffpa_attn_fp8_codes``), the pre-pass alone and ``ffpa_attn_func`` — every arm captured into a HIP graph of ``--iters`` calls, the arms replayed
INTERLEAVED, each twice per round, the median of the rounds reported; TFLOP/s on the dense (or causal) FLOP count, against the e4m3 MFMA peak for the FP8 arms.

  python tools/gpu_fwd_fp8_ab.py [--rounds 5] [--iters 10] [--json out.json]"""

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ffpa_attn_amd import attention_fwd_flops, ffpa_attn_fp8_codes, ffpa_attn_fp8_func, ffpa_attn_func, hip  # noqa: E402

E4M3_PEAK_TFLOPS = 5033.0  # MI355X dense e4m3 MFMA peak (2 x the bf16 peak of 2516)
SHAPES = {  # name -> (B, Hq, Hkv, Nq, Nkv, D, causal)
  "cfg2": (1, 32, 32, 8192, 8192, 512, False),
  "cfg2 causal": (1, 32, 32, 8192, 8192, 512, True),
  "cfg2 gqa 32:8": (1, 32, 8, 8192, 8192, 512, False),
  "D320": (1, 32, 32, 8192, 8192, 320, False),
  "cross Nq1024": (1, 32, 32, 1024, 8192, 512, False),
}


def graph_of(fn, iters):
  side = torch.cuda.Stream()
  with torch.cuda.stream(side):
    fn()
  torch.cuda.current_stream().wait_stream(side)
  torch.cuda.synchronize()
  g = torch.cuda.CUDAGraph()
  with torch.cuda.graph(g):
    for _ in range(iters):
      fn()
  return g


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--rounds", type=int, default=5)
  ap.add_argument("--iters", type=int, default=10)
  ap.add_argument("--json", default=None)
  args = ap.parse_args()
  rows = []
  for name, (B, hq, hkv, nq, nkv, D, causal) in SHAPES.items():
    torch.manual_seed(0)
    q = torch.randn(B, hq, nq, D, dtype=torch.bfloat16, device="cuda")
    k, v = (torch.randn(B, hkv, nkv, D, dtype=torch.bfloat16, device="cuda") for _ in range(2))
    scratch = hip.fp8_quantize(q, k, v, D ** -0.5 * 1.4426950408889634, True)
    arms = {
      "bf16": lambda: ffpa_attn_func(q, k, v, is_causal=causal, enable_gqa=True),
      "fp8 call": lambda: ffpa_attn_fp8_func(q, k, v, is_causal=causal, enable_gqa=True),
      "fp8 kernel": lambda: ffpa_attn_fp8_codes(*scratch, seqlen_q=nq, seqlen_kv=nkv, is_causal=causal),
      "fp8 pre-pass": lambda: hip.fp8_quantize(q, k, v, D ** -0.5 * 1.4426950408889634, True),
    }
    graphs = {a: graph_of(f, args.iters) for a, f in arms.items()}
    times = {a: [] for a in arms}
    for _ in range(args.rounds):
      for a in list(arms) * 2:  # interleaved, each arm twice per round
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        graphs[a].replay()
        end.record()
        end.synchronize()
        times[a].append(start.elapsed_time(end) / args.iters)
    flops = attention_fwd_flops(B, hq, nq, nkv, D, causal=causal)
    ms = {a: statistics.median(t) for a, t in times.items()}
    row = {"shape": name, **{f"{a} ms": round(ms[a], 4) for a in arms}, "bf16 TFLOP/s": round(flops / ms["bf16"] / 1e9, 1),
           "fp8 call TFLOP/s": round(flops / ms["fp8 call"] / 1e9, 1), "fp8 kernel TFLOP/s": round(flops / ms["fp8 kernel"] / 1e9, 1),
           "fp8 kernel / e4m3 peak": round(flops / ms["fp8 kernel"] / 1e9 / E4M3_PEAK_TFLOPS, 3), "bf16 / fp8 call": round(ms["bf16"] / ms["fp8 call"], 3)}
    rows.append(row)
    print(json.dumps(row), flush=True)
  if args.json:
    with open(args.json, "w") as f:
      json.dump(rows, f, indent=1)


if __name__ == "__main__":
  main()
