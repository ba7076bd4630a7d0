"""Developer tool: what the tree-mask latent call costs against the routes a caller had before it (profiles/r20_mla_tree.md).

  python tools/gpu_mla_tree_ab.py [--out profiles/r20_mla_tree.json] [--rounds 7] [--iters 20]
        arms per shape on the SAME tensors, interleaved, warmed, by graph replay:
          (tree)   ffpa_attn_with_kvcache_mla_tree(q, pool, 512, tree_mask=words): one launch over the draft tree;
          (tree2)  the same arm again, as an arm of its own in the same rounds: tree2 / tree is the run-to-run spread the ratios are read against;
          (causal) ffpa_attn_with_kvcache_mla(q, pool, 512, causal=True) on the same tensors: it walks the same tiles — a chain, not the tree: the cost floor;
          (paths)  one causal latent call per root-to-leaf path (q rows of the path's nodes, the prefix + the path's depth as the length), all in one graph: what a
                   caller that needs the tree's numbers from the causal call pays — the latent prefix streamed once per path.  The path's rows are NOT moved to the
                   cache's end first, so the figure is a lower bound of that route (its results are not the tree's: cost only);
          (two)    ffpa_attn_with_kvcache_tree(q, pool, pool)[..., :512] on the aliased pool: the two-cache kernel.
        Writes the records as JSON and a markdown table next to it.

Shapes: B = 32 sequences, page size 64, one latent head, Hq 16 and Hq 128, 1k / 4k / 16k rows per sequence (draft nodes included), a 16-node and a 64-node draft
tree (node i's parent is (i - 1) // 2: 8 / 32 root-to-leaf paths of depth 4 ... 5 / 6 ... 7), D = 576, head_dim_v = 512, bf16, scale 1 / sqrt(192).  Every figure is
the median of `--rounds` interleaved rounds of up to `--iters` replays each (fewer for an arm whose replay is long: `interleaved`), timed with device events."""

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

B, PAGE, D, DV = 32, 64, 576, 512
SCALE = 192 ** -0.5
SHAPES = [(hq, rows, nodes) for hq in (16, 128) for rows in (1024, 4096, 16384) for nodes in (16, 64)]


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


def interleaved(arms: dict, rounds, iters, round_ms=40.0):
  """Median / min / max per arm over `rounds` interleaved rounds.  An arm's round is `iters` replays, fewer where one replay is long: about `round_ms` of replays, at
  least two (the slow arms cost tens of milliseconds a replay: 20 of them per round would spend the run on the arm that needs the least resolution)."""
  n = {}
  for k, run in arms.items():  # warm-up, and the arm's replays per round
    once = time_us(run, 2)
    n[k] = max(2, min(iters, int(round_ms * 1e3 / max(once, 1e-3))))
    time_us(run, n[k])
  samples = {k: [] for k in arms}
  for _ in range(rounds):
    for k, run in arms.items():
      samples[k].append(time_us(run, n[k]))
  return {k: (statistics.median(v), min(v), max(v), n[k]) for k, v in samples.items()}


def tree_paths(nodes):
  """The draft tree (parent of node i: (i - 1) // 2) -> (bool mask [nodes, nodes]: a node sees its ancestors and itself, the node lists of its root-to-leaf paths)."""
  parents = [-1] + [(i - 1) // 2 for i in range(1, nodes)]
  mask = torch.zeros((nodes, nodes), dtype=torch.bool)
  for i in range(nodes):
    j = i
    while j >= 0:
      mask[i, j] = True
      j = parents[j]
  leaves = [i for i in range(nodes) if i not in set(parents)]
  return mask, [[int(j) for j in mask[leaf].nonzero().flatten()] for leaf in leaves]


def write_md(path, records):
  rows = ["| Hq | rows | nodes | paths | tree us | causal us | paths us | two-cache us | tree / causal | paths / tree | two-cache / tree | tree2 / tree (spread) | plan (tree) | plan (causal) |",
          "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
  for r in records:
    rows.append(f"| {r['Hq']} | {r['rows']} | {r['nodes']} | {r['paths']} | {r['tree_us']} | {r['causal_us']} | {r['paths_us']} | {r['two_us']} | {r['tree_over_causal']} | "
                f"{r['paths_over_tree']} | {r['two_over_tree']} | {r['tree2_over_tree']} | {r['plan_tree']} | {r['plan_causal']} |")
  with open(path, "w") as f:
    f.write("\n".join(rows) + "\n")


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--rounds", type=int, default=7)
  ap.add_argument("--iters", type=int, default=20)
  ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r20_mla_tree.json"))
  args = ap.parse_args()
  from ffpa_attn_amd import ffpa_attn_with_kvcache_mla, ffpa_attn_with_kvcache_mla_tree, ffpa_attn_with_kvcache_tree, hip, pack_tree_mask

  assert torch.cuda.is_available(), "needs a GPU"
  records = []
  for hq, rows, nodes in SHAPES:
    g = torch.Generator(device="cuda").manual_seed(rows + hq + nodes)
    pps = rows // PAGE
    pool = torch.empty((B * pps, PAGE, 1, D), device="cuda", dtype=torch.bfloat16).normal_(generator=g)
    table = torch.randperm(B * pps, generator=g, device="cuda").to(torch.int32).view(B, pps)
    q = torch.randn((B, nodes, hq, D), generator=g, device="cuda", dtype=torch.bfloat16)
    lens = torch.full((B,), rows, dtype=torch.int32, device="cuda")
    mask, paths = tree_paths(nodes)
    words = pack_tree_mask(mask.cuda())
    path_q = [q[:, p].contiguous() for p in paths]
    path_lens = [torch.full((B,), rows - nodes + len(p), dtype=torch.int32, device="cuda") for p in paths]

    tree = lambda: ffpa_attn_with_kvcache_mla_tree(q, pool, DV, tree_mask=words, cache_seqlens=lens, block_table=table, softmax_scale=SCALE)
    causal = lambda: ffpa_attn_with_kvcache_mla(q, pool, DV, cache_seqlens=lens, block_table=table, softmax_scale=SCALE, causal=True)
    two = lambda: ffpa_attn_with_kvcache_tree(q, pool, pool, cache_seqlens=lens, block_table=table, tree_mask=words, softmax_scale=SCALE)[..., :DV]

    def by_paths():
      return [ffpa_attn_with_kvcache_mla(pq, pool, DV, cache_seqlens=pl, block_table=table, softmax_scale=SCALE, causal=True) for pq, pl in zip(path_q, path_lens)]

    torch.testing.assert_close(tree().float(), two().float(), atol=2e-2, rtol=2e-2)  # (the two tree routes compute the same thing)
    plans = {}
    real_mla, real_tree = hip.mla_forward, hip.mla_tree_forward

    def spy_tree(*a, **kw):
      kw["plan_out"] = plans.setdefault("tree", {})
      return real_tree(*a, **kw)

    def spy_mla(*a, **kw):
      if kw.get("tree_words") is None:
        kw["plan_out"] = plans.setdefault("causal", {})
      return real_mla(*a, **kw)

    hip.mla_tree_forward, hip.mla_forward = spy_tree, spy_mla
    try:
      tree()
      causal()
    finally:
      hip.mla_tree_forward, hip.mla_forward = real_tree, real_mla
    brief = lambda p: f"{p['workgroups']} wg, {p['row_tiles']} row tiles, {p['splits']} splits{', NT' if ', NT>' in p['kernel'] else ''}"
    arms = {"tree": graphed(tree), "causal": graphed(causal), "paths": graphed(by_paths), "two": graphed(two), "tree2": graphed(tree)}
    r = interleaved(arms, args.rounds, args.iters)
    us = lambda k: round(r[k][0], 2)
    ratio = lambda a, b, nd=3: round(r[a][0] / r[b][0], nd)
    rec = {"Hq": hq, "B": B, "rows": rows, "nodes": nodes, "paths": len(paths), "tree_us": us("tree"), "tree2_us": us("tree2"), "causal_us": us("causal"),
           "paths_us": us("paths"), "two_us": us("two"), "tree_over_causal": ratio("tree", "causal"), "paths_over_tree": ratio("paths", "tree", 2),
           "two_over_tree": ratio("two", "tree", 2), "tree2_over_tree": ratio("tree2", "tree", 4), "min_max": {k: [round(x, 2) for x in v[1:3]] for k, v in r.items()}, "replays_per_round": {k: v[3] for k, v in r.items()},
           "latent_mib": round(B * rows * D * 2 / 2 ** 20, 1), "plan_tree": brief(plans["tree"]), "plan_causal": brief(plans["causal"])}
    records.append(rec)
    print(json.dumps(rec), flush=True)
    del pool, table, q, arms, path_q
    torch.cuda.empty_cache()
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, "w") as f:
    json.dump({"tool": "tools/gpu_mla_tree_ab.py", "rounds": args.rounds, "iters": args.iters, "records": records}, f, indent=1)
  write_md(os.path.splitext(args.out)[0] + "_table.md", records)


if __name__ == "__main__":
  main()
