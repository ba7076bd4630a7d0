"""Developer tool: the sparse and the tree-mask latent call over an FP8 pool against their 16-bit twins and against the route a caller had before them
(profiles/r24_mla_fp8_sparse_tree.md).  A measurement, not a gate.

  python tools/gpu_mla_fp8_sparse_tree_ab.py [--out profiles/r24_mla_fp8_sparse_tree.json] [--rounds 7] [--iters 20] [--only sparse|tree]
        arms per shape on the same q, indices / mask words, table and lengths, interleaved, warmed, by graph replay:
          (A)  the new call on the FP8 pool (OCP e4m3 codes, one byte per element, kv_scale = 0.5);
          (B)  the 16-bit twin on the dequantised pool, ``pool8.to(bf16)`` made ONCE outside the timed region, under softmax_scale * 0.5;
          (B') arm (B) again, as an arm of its own in the same rounds: B' / B is the run-to-run spread every ratio is read against;
          (C)  the route a caller has without the new calls, all of it inside the graph: dequantise the rows the step needs into a 16-bit scratch pool — the
               T x topk gathered rows of a sparse step (then a call with identity indices), the pages of every sequence of a tree step — and call the 16-bit twin.
        Writes the records as JSON and a markdown table next to it.

Shapes (profiles/r19_mla_sparse.md's and profiles/r20_mla_tree.md's).  Sparse: T = 32 tokens x topk 2048, token t's slots drawn from its own 32k rows of a pool of
32 x 32k rows, Hq 16 / 128.  Tree: B 32, pages of 64 keys, Hq 16 / 128 x 1k / 4k / 16k rows per sequence x 16- / 64-node trees (random trees: a node sees its
ancestors).  D = 576, head_dim_v = 512, bf16 q, scale 1 / sqrt(192).  Bytes are ALGORITHMIC: rows read x 576 B for the FP8 pool, twice that for the bf16 pool.
Every figure is the median of `--rounds` interleaved rounds of `--iters` replays each, timed with device events."""

import argparse
import json
import os
import random
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

B, PAGE, D, DV = 32, 64, 576, 512
SCALE = 192 ** -0.5
KV_SCALE = 0.5
SPARSE_SHAPES = [(hq, 32, 2048, 32768) for hq in (16, 128)]  # (Hq, tokens, topk, rows per token's sequence)
TREE_SHAPES = [(hq, L, nodes) for hq in (16, 128) for L in (1024, 4096, 16384) for nodes in (16, 64)]  # (Hq, rows per sequence, draft nodes)


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


def plans_of(hip, name, calls):
  """The plans of ``calls`` (label -> thunk), read through ``plan_out`` of ``hip.<name>``."""
  plans, real = {}, getattr(hip, name)
  for label, fn in calls.items():
    plan = plans[label] = {}
    setattr(hip, name, lambda *a, _p=plan, **kw: real(*a, **dict(kw, plan_out=_p)))
    try:
      fn()
    finally:
      setattr(hip, name, real)
  brief = lambda p: f"{p['workgroups']} wg, {p['row_tiles']} row tiles, {p['splits']} splits{', NT' if ', NT>' in p['kernel'] else ''}"
  return {k: brief(v) for k, v in plans.items()}


def record(kind, shape, r, rows_read, plans):
  a, b, b2, c = (r[k][0] for k in ("A", "B", "B'", "C"))
  return dict(kind=kind, **shape, A_us=round(a, 2), B_us=round(b, 2), Bb_us=round(b2, 2), C_us=round(c, 2), B_over_A=round(b / a, 3), C_over_A=round(c / a, 3),
              Bb_over_B=round(b2 / b, 4), A_min_max=[round(x, 2) for x in r["A"][1:]], B_min_max=[round(x, 2) for x in r["B"][1:]],
              C_min_max=[round(x, 2) for x in r["C"][1:]], fp8_mib=round(rows_read * D / 2 ** 20, 1), bf16_mib=round(rows_read * D * 2 / 2 ** 20, 1),
              A_tbs=round(rows_read * D / a / 1e6, 3), B_tbs=round(rows_read * D * 2 / b / 1e6, 3), plan_A=plans["A"], plan_B=plans["B"])


def sparse_records(args):
  from ffpa_attn_amd import ffpa_attn_with_kvcache_mla_sparse, ffpa_attn_with_kvcache_mla_sparse_fp8, hip, quantize_latent_rows

  out = []
  for hq, T, topk, per in SPARSE_SHAPES:
    g = torch.Generator(device="cuda").manual_seed(0)
    rows = T * per
    pool8 = torch.empty((rows, 1, D), dtype=torch.float8_e4m3fn, device="cuda")
    for lo in range(0, rows, 1 << 16):  # (in slabs: the fp32 draw of the whole pool need not live at once)
      pool8[lo:lo + (1 << 16)] = quantize_latent_rows(torch.randn((min(1 << 16, rows - lo), 1, D), generator=g, device="cuda", dtype=torch.bfloat16), KV_SCALE)
    pool16 = pool8.to(torch.bfloat16)
    idx = torch.stack([t * per + torch.randperm(per, device="cuda", generator=g)[:topk] for t in range(T)]).to(torch.int32)
    q = torch.randn((T, hq, D), generator=g, device="cuda", dtype=torch.bfloat16)
    scratch = torch.empty((T * topk, 1, D), dtype=torch.bfloat16, device="cuda")
    ident = torch.arange(T * topk, dtype=torch.int32, device="cuda").view(T, topk)
    flat = idx.flatten().to(torch.int64)
    new = lambda: ffpa_attn_with_kvcache_mla_sparse_fp8(q, pool8, DV, idx, kv_scale=KV_SCALE, softmax_scale=SCALE)
    wide = lambda: ffpa_attn_with_kvcache_mla_sparse(q, pool16, DV, idx, softmax_scale=SCALE * KV_SCALE)

    def today():
      scratch.copy_(pool8[flat])  # (gather + widen: one pass over the step's rows, one write of twice their bytes)
      return ffpa_attn_with_kvcache_mla_sparse(q, scratch, DV, ident, softmax_scale=SCALE * KV_SCALE)

    assert torch.equal(new(), wide() * KV_SCALE)  # (a power-of-two scale: the two routes return the same bits)
    torch.testing.assert_close(today().float(), wide().float(), atol=2e-2, rtol=2e-2)  # (the same rows in another place: the same attention)
    plans = plans_of(hip, "mla_sparse_forward", {"A": new, "B": wide})
    r = interleaved({"A": graphed(new), "B": graphed(wide), "B'": graphed(wide), "C": graphed(today)}, args.rounds, args.iters)
    rec = record("sparse", dict(Hq=hq, tokens=T, topk=topk, pool_rows=rows), r, T * topk, plans)
    out.append(rec)
    print(json.dumps(rec), flush=True)
    del pool8, pool16, scratch
    torch.cuda.empty_cache()
  return out


def tree_words(nodes, seed):
  from ffpa_attn_amd import pack_tree_mask

  rng = random.Random(seed)
  masks = []
  for _ in range(B):
    m = torch.eye(nodes, dtype=torch.bool)
    for i in range(1, nodes):
      m[i] |= m[rng.randrange(i)]  # (a random parent among the earlier nodes: node i sees its ancestors and itself)
    masks.append(m)
  return pack_tree_mask(torch.stack(masks).cuda())


def tree_records(args):
  from ffpa_attn_amd import ffpa_attn_with_kvcache_mla_tree, ffpa_attn_with_kvcache_mla_tree_fp8, hip, quantize_latent_rows

  out = []
  for hq, L, nodes in TREE_SHAPES:
    g = torch.Generator(device="cuda").manual_seed(0)
    pps = L // PAGE
    n_pages = B * pps
    pool8 = quantize_latent_rows(torch.randn((n_pages, PAGE, 1, D), generator=g, device="cuda", dtype=torch.bfloat16), KV_SCALE)
    pool16 = pool8.to(torch.bfloat16)
    table = torch.randperm(n_pages, device="cuda", generator=g).to(torch.int32).view(B, pps)
    q = torch.randn((B, nodes, hq, D), generator=g, device="cuda", dtype=torch.bfloat16)
    lens = torch.full((B,), L, dtype=torch.int32, device="cuda")  # (the draft rows are the last `nodes` rows of every sequence: already in the cache)
    words = tree_words(nodes, nodes)
    scratch = torch.empty_like(pool16)
    new = lambda: ffpa_attn_with_kvcache_mla_tree_fp8(q, pool8, DV, kv_scale=KV_SCALE, tree_mask=words, cache_seqlens=lens, block_table=table, softmax_scale=SCALE)
    wide = lambda: ffpa_attn_with_kvcache_mla_tree(q, pool16, DV, tree_mask=words, cache_seqlens=lens, block_table=table, softmax_scale=SCALE * KV_SCALE)

    def today():
      scratch.copy_(pool8)  # (every page of every sequence of the step, widened: one read of the pool, one write of twice its bytes)
      return ffpa_attn_with_kvcache_mla_tree(q, scratch, DV, tree_mask=words, cache_seqlens=lens, block_table=table, softmax_scale=SCALE * KV_SCALE)

    assert torch.equal(new(), wide() * KV_SCALE)
    assert torch.equal(today(), wide())  # (the same call on a copy of the same pool)
    plans = plans_of(hip, "mla_forward", {"A": new, "B": wide})
    r = interleaved({"A": graphed(new), "B": graphed(wide), "B'": graphed(wide), "C": graphed(today)}, args.rounds, args.iters)
    rec = record("tree", dict(Hq=hq, B=B, L=L, nodes=nodes), r, B * L, plans)
    out.append(rec)
    print(json.dumps(rec), flush=True)
    del pool8, pool16, scratch, table, q
    torch.cuda.empty_cache()
  return out


def write_md(path, records):
  rows = ["| call | Hq | shape | A: fp8 us | B: bf16 us | C: dequantise + bf16 us | B / A | C / A | B' / B (spread) | fp8 MiB | bf16 MiB | A TB/s | B TB/s | plan (A) | plan (B) |",
          "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
  for r in records:
    shape = f"T {r['tokens']} x topk {r['topk']} of {r['pool_rows']} rows" if r["kind"] == "sparse" else f"B {r['B']} x {r['L']} rows, {r['nodes']} nodes"
    rows.append(f"| {r['kind']} | {r['Hq']} | {shape} | {r['A_us']} | {r['B_us']} | {r['C_us']} | {r['B_over_A']} | {r['C_over_A']} | {r['Bb_over_B']} | {r['fp8_mib']} | "
                f"{r['bf16_mib']} | {r['A_tbs']} | {r['B_tbs']} | {r['plan_A']} | {r['plan_B']} |")
  with open(path, "w") as f:
    f.write("\n".join(rows) + "\n")


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--rounds", type=int, default=7)
  ap.add_argument("--iters", type=int, default=20)
  ap.add_argument("--only", choices=("sparse", "tree"), default=None)
  ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r24_mla_fp8_sparse_tree.json"))
  args = ap.parse_args()
  assert torch.cuda.is_available(), "needs a GPU"
  records = []
  if args.only != "tree":
    records += sparse_records(args)
  if args.only != "sparse":
    records += tree_records(args)
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, "w") as f:
    json.dump({"tool": "tools/gpu_mla_fp8_sparse_tree_ab.py", "rounds": args.rounds, "iters": args.iters, "kv_scale": KV_SCALE, "records": records}, f, indent=1)
  write_md(os.path.splitext(args.out)[0] + "_table.md", records)


if __name__ == "__main__":
  main()
