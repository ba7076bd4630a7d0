"""Developer tool: what the sliding-window call saves on a decode step, and whether the existing launches kept their speed (profiles/r13_window.{json,md}).

  python tools/gpu_window_ab.py window [--out profiles/r13_window.json]
        three arms per shape and window, interleaved, warmed, in graph replay and eager:
          (a) ffpa_attn_with_kvcache_window(window_size=(left, 0)) over the 32k cache;
          (b) ffpa_attn_with_kvcache(causal=True) over the same 32k cache — what a caller pays today, short of the dense-mask route;
          (c) ffpa_attn_with_kvcache(causal=True) over a cache that holds only left + 1 keys — the ideal;
          (c2) arm (c) again, as an arm of its own in the same rounds: c2 / c is the run-to-run spread the ratios are read against.
        Writes the records as JSON and a markdown table next to it.
  python tools/gpu_window_ab.py causal --lib PATH --tag T
        the plain causal decode launch alone with the library at PATH (one process per library: run it for the parent commit's build and for this one
        alternately — and each twice: the spread — and compare the lines; a saved build of the parent lacks the window symbols: it is loaded by path, which
        binds what it has)

Batch: the bench's varlen_decode family — 32 sequences x 1 token, paged (page 64), L = 32768 keys each, GQA 32 / 8 at D 512 and 16 / 4 at D 1024; left in
1k / 4k / 16k.  Every figure is the median of `--rounds` interleaved rounds of `--iters` launches each, timed with device events."""

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

B, PAGE, L = 32, 64, 32768
SHAPES = [(512, (32, 8)), (1024, (16, 4))]
LEFTS = [1024, 4096, 16384]


def batch(d, heads, seed=0):
  g = torch.Generator(device="cuda").manual_seed(seed)
  hq, hkv = heads
  pps = L // PAGE
  n_pages = B * pps
  kc = torch.randn((n_pages, PAGE, hkv, d), generator=g, device="cuda", dtype=torch.bfloat16)
  vc = torch.randn((n_pages, PAGE, hkv, d), generator=g, device="cuda", dtype=torch.bfloat16)
  table = torch.randperm(n_pages, device="cuda", generator=g).to(torch.int32).view(B, pps)
  q = torch.randn((B, 1, hq, d), generator=g, device="cuda", dtype=torch.bfloat16)
  return q, kc, vc, table


def graphed(fn):
  side = torch.cuda.Stream()
  side.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(side):
    for _ in range(3):
      fn()
  torch.cuda.current_stream().wait_stream(side)
  g = torch.cuda.CUDAGraph()
  with torch.cuda.graph(g):
    fn()
  return g.replay


def time_us(run, iters):
  start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  start.record()
  for _ in range(iters):
    run()
  end.record()
  torch.cuda.synchronize()
  return start.elapsed_time(end) * 1e3 / iters


def interleaved(arms: dict, rounds, iters):
  for run in arms.values():  # warm-up
    time_us(run, iters)
  samples = {k: [] for k in arms}
  for _ in range(rounds):
    for k, run in arms.items():
      samples[k].append(time_us(run, iters))
  return {k: (statistics.median(v), min(v), max(v)) for k, v in samples.items()}


def write_md(path, records):
  rows = ["| D | heads | left | mode | (a) window us | (b) causal 32k us | (c) causal left+1 us | a / b | a / c | c2 / c (spread) | plan (a) | plan (c) |",
          "|---|---|---|---|---|---|---|---|---|---|---|---|"]
  for r in records:
    rows.append(f"| {r['D']} | {r['heads'][0]} / {r['heads'][1]} | {r['left']} | {r['mode']} | {r['a_us']} | {r['b_us']} | {r['c_us']} | {r['a_over_b']} | {r['a_over_c']} | "
                f"{r['c2_over_c']} | {r['plan_a']} | {r['plan_c']} |")
  with open(path, "w") as f:
    f.write("\n".join(rows) + "\n")


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("mode", choices=["window", "causal"])
  ap.add_argument("--lib", default=None)
  ap.add_argument("--tag", default="this build")
  ap.add_argument("--rounds", type=int, default=7)
  ap.add_argument("--iters", type=int, default=30)
  ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r13_window.json"))
  args = ap.parse_args()
  from ffpa_attn_amd import ffpa_attn_with_kvcache, hip

  if args.lib:
    hip._lib = hip.load_library(os.path.abspath(args.lib))  # (by path: a saved build of an older commit binds the symbols it has)
  assert torch.cuda.is_available(), "needs a GPU"
  full = torch.full((B,), L, dtype=torch.int32, device="cuda")
  if args.mode == "causal":
    for d, heads in SHAPES:
      q, kc, vc, table = batch(d, heads)
      fn = lambda: ffpa_attn_with_kvcache(q, kc, vc, cache_seqlens=full, block_table=table, causal=True)
      for mode, run in (("graph", graphed(fn)), ("eager", fn)):
        med, lo, hi = interleaved({"causal": run}, args.rounds, args.iters)["causal"]
        print(json.dumps({"mode": "causal " + mode, "tag": args.tag, "D": d, "heads": heads, "L": L, "median_us": round(med, 2), "min_us": round(lo, 2),
                          "max_us": round(hi, 2)}), flush=True)
      del q, kc, vc, table
    return
  from ffpa_attn_amd import ffpa_attn_with_kvcache_window

  records = []
  for d, heads in SHAPES:
    q, kc, vc, table = batch(d, heads)
    for left in LEFTS:
      short = torch.full((B,), left + 1, dtype=torch.int32, device="cuda")
      short_table = table[:, :-(-(left + 1) // PAGE)]  # (a cache of left + 1 keys: the plan sees that capacity)
      # the window call over the long cache and the causal call over the short one attend to the same keys only if the short cache holds the LAST left + 1
      # keys; the timing does not depend on which pages those are, so arm (c) reads the first ones
      fa = lambda: ffpa_attn_with_kvcache_window(q, kc, vc, cache_seqlens=full, block_table=table, window_size=(left, 0))
      fb = lambda: ffpa_attn_with_kvcache(q, kc, vc, cache_seqlens=full, block_table=table, causal=True)
      fc = lambda: ffpa_attn_with_kvcache(q, kc, vc, cache_seqlens=short, block_table=short_table, causal=True)
      plan_a = hip.varlen_launch_plan(B, heads[0], heads[1], 1, L, d, causal=True, total_q=B, page_size=PAGE, window=(left, 0))
      plan_c = hip.varlen_launch_plan(B, heads[0], heads[1], 1, short_table.size(1) * PAGE, d, causal=True, total_q=B, page_size=PAGE)
      brief = lambda p: f"{p['splits']} splits{', NT' if ', NT>' in p['kernel'] else ''}"
      for mode, arms in (("graph", {"a": graphed(fa), "b": graphed(fb), "c": graphed(fc), "c2": graphed(fc)}), ("eager", {"a": fa, "b": fb, "c": fc, "c2": fc})):
        r = interleaved(arms, args.rounds, args.iters)
        rec = {"D": d, "heads": list(heads), "B": B, "L": L, "left": left, "mode": mode, "a_us": round(r["a"][0], 2), "b_us": round(r["b"][0], 2),
               "c_us": round(r["c"][0], 2), "c2_us": round(r["c2"][0], 2), "a_over_b": round(r["a"][0] / r["b"][0], 4), "a_over_c": round(r["a"][0] / r["c"][0], 4),
               "c2_over_c": round(r["c2"][0] / r["c"][0], 4), "a_min_max": [round(x, 2) for x in r["a"][1:]], "c_min_max": [round(x, 2) for x in r["c"][1:]],
               "plan_a": brief(plan_a), "plan_c": brief(plan_c)}
        records.append(rec)
        print(json.dumps(rec), flush=True)
    del q, kc, vc, table
    torch.cuda.empty_cache()
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, "w") as f:
    json.dump({"tool": "tools/gpu_window_ab.py window", "rounds": args.rounds, "iters": args.iters, "records": records}, f, indent=1)
  write_md(os.path.splitext(args.out)[0] + "_table.md", records)


if __name__ == "__main__":
  main()
