"""Developer tool: shared-prefix (cascade) attention over the MLA latent cache against the plain latent call (profiles/r26_mla_cascade.md).

  python tools/gpu_mla_cascade_ab.py [--out profiles/r26_mla_cascade.json] [--rounds 5] [--iters 10] [--grid fit|full|check]
        per shape, on the SAME tensors, interleaved, warmed:
          (cascade)  ffpa_attn_with_kvcache_mla_cascade(..., cascade=True): plan + prefix pass + suffix pass + merge, replayed from one HIP graph;
          (plain)    ffpa_attn_with_kvcache_mla(...): the one launch there was, replayed from a graph;
          (plain2)   arm (plain) again, as an arm of its own in the same rounds: plain2 / plain is the run-to-run spread the ratio is read against;
          (cascade eager) / (plain eager): the same two calls launched from Python.
        and, once per run, the plan kernel's own time against the torch route it replaces (about ten small launches), both replayed from a graph.

Shapes ("fit"): Hq 16 and 128 on one latent head; B 16 and 64 as one group, and B 64 as 8 groups of 8; shared prefixes of 2k, 8k and 32k keys; suffixes of 128
and 2k keys per sequence ("full" adds 512); 1 token, and 4 tokens causal; pages of 64; bf16 — plus one FP8 row.  "check": shapes OFF that grid (B 8 ... 256, prefixes of
4k ... 64k, pages of 128, groups of 4 ... 96, other suffixes), for the rule fitted to the grid: what it takes and its near misses.  D = 576, head_dim_v = 512, scale 1 / sqrt(192).  Every figure is the median
of `--rounds` interleaved rounds of `--iters` runs each, timed with device events.  Bytes are ALGORITHMIC: latent rows x 1152 B, every row once per reader."""

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

D, DV = 576, 512
SCALE = 192 ** -0.5


def shapes(grid):
  """(Hq, B, G, P, suffix, Sq, page, fp8)"""
  out = []
  if grid in ("fit", "full"):
    sufs = (128, 512, 2048) if grid == "full" else (128, 2048)
    for hq in (16, 128):
      for B, G in ((16, 1), (64, 1), (64, 8)):
        for P in (2048, 8192, 32768):
          for s in sufs:
            for sq in (1, 4):
              out.append((hq, B, G, P, s, sq, 64, False))
    out.append((16, 64, 8, 8192, 128, 1, 64, True))
  else:
    for hq in (16, 128):
      for B, G, P, s, sq, page in ((32, 1, 4096, 512, 1, 64), (32, 4, 16384, 512, 1, 128), (32, 4, 4096, 512, 4, 64), (32, 1, 16384, 512, 4, 128),
                                   (8, 1, 32768, 512, 1, 64), (128, 16, 2048, 512, 1, 64)):
        out.append((hq, B, G, P, s, sq, page, False))
    # around the fitted rule (Hq 16, one token, B x P >= 2^21 sequence-keys, 8 or more sequences per group): shapes it takes, off the grid in B, P, the group size
    # and the page — and its near misses at half the sequence-keys, or 4 sequences per group
    for B, G, P, s, page, fp8 in ((128, 16, 16384, 512, 64, False), (96, 1, 24576, 300, 128, False), (32, 2, 65536, 1000, 64, False), (256, 8, 8192, 512, 128, False),
                                  (64, 8, 32768, 128, 64, True), (64, 8, 16384, 512, 64, False), (128, 16, 8192, 512, 64, False), (64, 16, 32768, 512, 64, False)):
      out.append((16, B, G, P, s, 1, page, fp8))
  return out


def batch(hq, B, G, P, suffix, sq, page, fp8, seed=0):
  """G groups of B / G sequences; every group's P shared keys are the same pages in the rows of its sequences; every sequence has `suffix` keys of its own."""
  g = torch.Generator(device="cuda").manual_seed(seed)
  npre, own = P // page, -(-(suffix + sq) // page)
  W = npre + own
  n_pages = G * npre + B * own
  ids = torch.randperm(n_pages, device="cuda", generator=g).to(torch.int32)
  table = torch.empty((B, W), dtype=torch.int32, device="cuda")
  per = B // G
  for b in range(B):
    table[b, :npre] = ids[(b // per) * npre:(b // per + 1) * npre]
    table[b, npre:] = ids[G * npre + b * own:G * npre + (b + 1) * own]
  kv = torch.randn((n_pages, page, 1, D), generator=g, device="cuda", dtype=torch.bfloat16)
  if fp8:
    kv = kv.to(torch.float8_e4m3fn)
  q = torch.randn((B, sq, hq, D), generator=g, device="cuda", dtype=torch.bfloat16)
  lens = torch.full((B,), P + suffix, dtype=torch.int32, device="cuda")
  cu = torch.arange(0, B + 1, per, dtype=torch.int32, device="cuda")
  spl = torch.full((G,), P, dtype=torch.int32, device="cuda")
  return q, kv, table, lens, cu, spl, per


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
  return {k: statistics.median(v) for k, v in samples.items()}


def torch_plan(lens, table, cu, spl, page, sq, causal, cap):
  """The route the plan kernel replaces, in torch ops (the same outputs; nothing read back)."""
  B, W = table.shape
  G = cu.numel() - 1
  seq = torch.arange(B, device=lens.device)
  grp = torch.searchsorted(cu[1:].contiguous(), seq.to(torch.int32), right=True).clamp(max=G - 1)
  held = lens.clamp(0, cap)
  floor_ = torch.full((G,), cap, dtype=torch.int32, device=lens.device).scatter_reduce(0, grp, held - (sq - 1 if causal else 0), "amin")
  P = torch.minimum(spl, floor_).clamp(0, cap) // page * page
  first = cu[:-1].clamp(max=B - 1).long()
  cols = (torch.arange(W, device=lens.device)[None, :] + (P[grp] // page)[:, None]).clamp(max=W - 1)
  return cu * sq, P, table[first], torch.gather(table, 1, cols), held - P[grp]


def write_md(path, records, plan):
  rows = ["| Hq | B | groups | prefix | suffix | tokens | page | pool | cascade us | plain us | plain / cascade | eager: cascade us | plain us | plain / cascade | "
          "plain2 / plain | plain MiB | cascade MiB | rule |", "|" + "---|" * 18]
  for r in records:
    rows.append(f"| {r['Hq']} | {r['B']} | {r['G']} | {r['P']} | {r['suffix']} | {r['Sq']} | {r['page']} | {'fp8' if r['fp8'] else 'bf16'} | {r['us']['cascade']} | "
                f"{r['us']['plain']} | {r['speedup']} | {r['us']['cascade eager']} | {r['us']['plain eager']} | {r['speedup_eager']} | {r['spread']} | "
                f"{r['plain_mib']} | {r['cascade_mib']} | {'cascade' if r['rule'] else 'plain'} |")
  rows.append("")
  rows.append(f"Plan launch (B {plan['B']}, {plan['G']} groups, {plan['W']} pages per sequence, replayed from a graph): kernel {plan['kernel_us']} us, "
              f"the torch route it replaces {plan['torch_us']} us.")
  with open(path, "w") as f:
    f.write("\n".join(rows) + "\n")


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--rounds", type=int, default=5)
  ap.add_argument("--iters", type=int, default=10)
  ap.add_argument("--grid", default="fit", choices=("fit", "full", "check"))
  ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r26_mla_cascade.json"))
  args = ap.parse_args()
  from ffpa_attn_amd import (ffpa_attn_with_kvcache_mla, ffpa_attn_with_kvcache_mla_cascade, ffpa_attn_with_kvcache_mla_cascade_fp8, ffpa_attn_with_kvcache_mla_fp8,
                             hip, mla_cascade_rule)

  hip.load_library()  # (and the ffpa_attn ops are registered)

  assert torch.cuda.is_available(), "needs a GPU"
  # the plan launch on its own, against the torch ops it replaces
  q, kv, table, lens, cu, spl, per = batch(16, 64, 8, 8192, 128, 1, 64, False)
  cap = table.size(1) * 64
  kernel = lambda: torch.ops.ffpa_attn._mla_cascade_plan_hip(lens, table, cu, spl, 0, 64, 1, 0, cap)
  route = lambda: torch_plan(lens, table, cu, spl, 64, 1, False, cap)
  for a, b in zip(kernel(), route()):
    assert torch.equal(a, b.to(torch.int32))
  r = interleaved({"kernel": graphed(kernel), "torch": graphed(route)}, args.rounds, 50)
  plan = {"B": 64, "G": 8, "W": table.size(1), "kernel_us": round(r["kernel"], 2), "torch_us": round(r["torch"], 2)}
  print(json.dumps(plan), flush=True)
  records = []
  for hq, B, G, P, suffix, sq, page, fp8 in shapes(args.grid):
    q, kv, table, lens, cu, spl, per = batch(hq, B, G, P, suffix, sq, page, fp8)
    causal = sq > 1
    kw = dict(cache_seqlens=lens, block_table=table, softmax_scale=SCALE, causal=causal)
    if fp8:
      kw["kv_scale"] = 0.5
    cas_fn, plain_fn = (ffpa_attn_with_kvcache_mla_cascade_fp8, ffpa_attn_with_kvcache_mla_fp8) if fp8 else (ffpa_attn_with_kvcache_mla_cascade, ffpa_attn_with_kvcache_mla)
    cascade = lambda: cas_fn(q, kv, DV, shared_prefix_len=spl, cu_group_seqs=cu, max_group_seqs=per, cascade=True, **kw)
    plain = lambda: plain_fn(q, kv, DV, **kw)
    torch.testing.assert_close(cascade().float(), plain().float(), atol=2e-2, rtol=2e-2)  # (the two routes compute the same thing)
    r = interleaved({"cascade": graphed(cascade), "plain": graphed(plain), "plain2": graphed(plain), "cascade eager": cascade, "plain eager": plain}, args.rounds,
                    args.iters)
    row = D * (1 if fp8 else 2)
    rec = {"Hq": hq, "Hkv": 1, "B": B, "G": G, "P": P, "suffix": suffix, "Sq": sq, "page": page, "fp8": fp8, "us": {k: round(v, 2) for k, v in r.items()},
           "speedup": round(r["plain"] / r["cascade"], 3), "speedup_eager": round(r["plain eager"] / r["cascade eager"], 3),
           "spread": round(r["plain2"] / r["plain"], 4), "plain_mib": round(B * (P + suffix) * row / 2 ** 20, 1),
           "cascade_mib": round((G * P + B * suffix) * row / 2 ** 20, 1), "rule": bool(mla_cascade_rule(B, sq, hq, 1, P, G))}
    records.append(rec)
    print(json.dumps(rec), flush=True)
    del q, kv, table
    torch.cuda.empty_cache()
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, "w") as f:
    json.dump({"tool": "tools/gpu_mla_cascade_ab.py", "grid": args.grid, "rounds": args.rounds, "iters": args.iters, "rows": records, "plan": plan}, f, indent=1)
  write_md(os.path.splitext(args.out)[0] + "_table.md", records, plan)


if __name__ == "__main__":
  main()
