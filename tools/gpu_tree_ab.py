"""Developer tool: what the tree mask costs, and whether the existing launches kept their speed (profiles/r12_tree_mask.md).

  python tools/gpu_tree_ab.py cost                         tree(tril) vs ffpa_attn_with_kvcache(causal=True), this build, interleaved, in graph replay
  python tools/gpu_tree_ab.py paths                        one causal call per root-to-leaf path of a 16-node, 4-leaf tree vs the one tree call
  python tools/gpu_tree_ab.py causal --lib PATH --tag T    the causal kvcache call alone with the library at PATH (one process per library: run it for
                                                           two builds alternately — and for the same build twice: the spread — and compare the lines)
  python tools/gpu_tree_ab.py bench --lib PATH --tag T -- --gpus 1 --steps 30 --warmup 5 --workload varlen_decode
                                                           bench.py in this process with the library at PATH (a saved build of the parent commit lacks the
                                                           tree symbols: it is loaded by path, which binds what it has); alternate the libraries as above

The order profiles/r12_tree_mask.md was taken in, every step under its own `timeout` and chained with `&&`: cost, paths, then causal and bench for
parent, this build, parent, this build (the two runs of a library are its A/A spread).

Batch: the bench's varlen_decode shape — 32 sequences, 1k ... 16k keys, paged (page 64), GQA 32 / 8 at D 512 and 16 / 4 at D 1024.  Every figure is the median of
`--rounds` interleaved rounds of `--iters` graph replays each, timed with device events; one JSON line per figure."""

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def batch(d, heads, sq, seed=0):
  g = torch.Generator(device="cuda").manual_seed(seed)
  hq, hkv = heads
  B, page = 32, 64
  lens = [1024 + (15 * 1024 * i) // (B - 1) for i in range(B)]
  pps = -(-max(lens) // page)
  n_pages = B * pps
  kc = torch.randn((n_pages, page, hkv, d), generator=g, device="cuda", dtype=torch.bfloat16)
  vc = torch.randn((n_pages, page, hkv, d), generator=g, device="cuda", dtype=torch.bfloat16)
  table = torch.randperm(n_pages, device="cuda", generator=g).to(torch.int32).view(B, pps)
  q = torch.randn((B, sq, hq, d), generator=g, device="cuda", dtype=torch.bfloat16)
  return q, kc, vc, torch.tensor(lens, dtype=torch.int32, device="cuda"), table


def graphed(fn):
  side = torch.cuda.Stream()
  side.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(side):
    for _ in range(3):
      fn()
  torch.cuda.current_stream().wait_stream(side)
  g = torch.cuda.CUDAGraph()
  with torch.cuda.graph(g):
    out = fn()
  return g, out


def time_us(g, iters):
  start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  start.record()
  for _ in range(iters):
    g.replay()
  end.record()
  torch.cuda.synchronize()
  return start.elapsed_time(end) * 1e3 / iters


def interleaved(graphs: dict, rounds, iters):
  for g in graphs.values():  # warm-up
    time_us(g, iters)
  samples = {k: [] for k in graphs}
  for _ in range(rounds):
    for k, g in graphs.items():
      samples[k].append(time_us(g, iters))
  return {k: (statistics.median(v), min(v), max(v)) for k, v in samples.items()}


SHAPES = [(512, (32, 8), 4), (512, (32, 8), 16), (1024, (16, 4), 4), (1024, (16, 4), 16)]


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("mode", choices=["cost", "paths", "causal", "bench"])
  ap.add_argument("--lib", default=None)
  ap.add_argument("--tag", default="this build")
  ap.add_argument("--rounds", type=int, default=7)
  ap.add_argument("--iters", type=int, default=50)
  args, rest = ap.parse_known_args()  # (bench mode: what follows `--` goes to bench.py)
  args.bench_args = [x for x in rest if x != "--"]
  from ffpa_attn_amd import ffpa_attn_with_kvcache, hip

  if args.lib:
    hip._lib = hip.load_library(os.path.abspath(args.lib))  # (by path: a saved build of an older commit binds the symbols it has)
  if args.mode == "bench":
    import runpy

    print(f"bench.py {' '.join(args.bench_args)} [{args.tag}]", flush=True)
    sys.argv = ["bench.py", *args.bench_args]
    runpy.run_path(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bench.py"), run_name="__main__")
    return

  assert torch.cuda.is_available(), "needs a GPU"
  if args.mode == "causal":
    for d, heads, sq in SHAPES:
      q, kc, vc, lens, table = batch(d, heads, sq)
      g, _ = graphed(lambda: ffpa_attn_with_kvcache(q, kc, vc, cache_seqlens=lens, block_table=table, causal=True))
      med, lo, hi = interleaved({"causal": g}, args.rounds, args.iters)["causal"]
      print(json.dumps({"mode": "causal", "tag": args.tag, "D": d, "heads": heads, "Sq": sq, "median_us": round(med, 2), "min_us": round(lo, 2), "max_us": round(hi, 2)}), flush=True)
    return
  from ffpa_attn_amd import ffpa_attn_with_kvcache_tree, pack_tree_mask

  if args.mode == "cost":
    for d, heads, sq in SHAPES:
      q, kc, vc, lens, table = batch(d, heads, sq)
      words = pack_tree_mask(torch.tril(torch.ones((sq, sq), dtype=torch.bool, device="cuda")))
      gc, oc = graphed(lambda: ffpa_attn_with_kvcache(q, kc, vc, cache_seqlens=lens, block_table=table, causal=True))
      gt, ot = graphed(lambda: ffpa_attn_with_kvcache_tree(q, kc, vc, cache_seqlens=lens, block_table=table, tree_mask=words))
      assert torch.equal(oc, ot), "tril(ones) is not the causal call's bits"
      r = interleaved({"causal": gc, "tree": gt}, args.rounds, args.iters)
      print(json.dumps({"mode": "cost", "D": d, "heads": heads, "Sq": sq, "causal_us": round(r["causal"][0], 2), "tree_us": round(r["tree"][0], 2),
                        "tree_over_causal": round(r["tree"][0] / r["causal"][0], 4), "causal_min_max": [round(x, 2) for x in r["causal"][1:]],
                        "tree_min_max": [round(x, 2) for x in r["tree"][1:]]}), flush=True)
    return
  # paths: a 16-node tree of 4 leaves (a root chain of 4, then 4 branches of 3).  A caller without the tree call runs one causal call per path, each on its own
  # copy of the path's 7 draft keys behind the prefix.  What is timed here are the four attention launches ALONE — 7 query tokens each, on the same cache: writing
  # each path's keys behind the prefix is not timed, so the figure is a LOWER bound of what that caller pays (every result line says so).
  parents = [-1, 0, 1, 2] + [3, 4, 5] + [3, 7, 8] + [3, 10, 11] + [3, 13, 14]
  mask = torch.zeros((16, 16), dtype=torch.bool)
  for i in range(16):
    j = i
    while j >= 0:
      mask[i, j] = True
      j = parents[j]
  for d, heads in ((512, (32, 8)), (1024, (16, 4))):
    q, kc, vc, lens, table = batch(d, heads, 16)
    words = pack_tree_mask(mask.cuda())
    gt, _ = graphed(lambda: ffpa_attn_with_kvcache_tree(q, kc, vc, cache_seqlens=lens, block_table=table, tree_mask=words))
    q7 = q[:, :7].contiguous()
    gp, _ = graphed(lambda: [ffpa_attn_with_kvcache(q7, kc, vc, cache_seqlens=lens, block_table=table, causal=True) for _ in range(4)])
    r = interleaved({"tree": gt, "paths": gp}, args.rounds, args.iters)
    print(json.dumps({"mode": "paths", "D": d, "heads": heads, "tree_call_us": round(r["tree"][0], 2), "four_causal_calls_us": round(r["paths"][0], 2),
                      "paths_over_tree": round(r["paths"][0] / r["tree"][0], 3),
                      "note": "attention launches only: the per-path copies of the draft keys are not timed (a lower bound for the per-path caller)"}), flush=True)


if __name__ == "__main__":
  main()
