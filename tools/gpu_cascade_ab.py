"""A/B of cascade (shared-prefix) attention against the plain paged launch on the same shared-page table, interleaved in one process (tools/gpu_ab.py's method:
alternating rounds, medians).  Every sequence of the batch points at the same P / page_size prefix pages, followed by pages of its own; the pool's pages are
SHUFFLED.  Both sides run ffpa_attn_with_kvcache_cascade — cascade=False (the plain launch: every (sequence, KV head) workgroup streams the prefix) and
cascade=True (prefix pass once for the batch + suffix pass + merge) — replayed from a captured HIP graph (a decode step's setting) and, as a second figure,
launched eagerly from Python.

  python tools/gpu_cascade_ab.py [--rounds 7] [--iters 20] [--quick] [--check] [--out FILE]

Workloads: D 512 GQA 32 / 8 and D 1024 GQA 16 / 4, page 64, B in {4, 16, 64}, Sq in {1, 4}, P in {2k, 8k, 32k} (the prefix's K + V straddles
the 256 MiB Infinity Cache), suffix lengths drawn from 128 ... 2048: the "grid" rows the cascade=None rule is fitted to.  --check measures the "check" rows instead:
D 512 at page 256 (GQA 32 / 8) and at a GQA group of 8 (64 / 8), on both sides of the rule's threshold.  The kernel times of the launches come from a separate
``rocprofv3 --kernel-trace --stats -- python tools/gpu_cascade_ab.py --quick`` run."""

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from ffpa_attn_amd import ffpa_attn_with_kvcache_cascade  # noqa: E402


def shared_case(B, P, suffix, page, hkv, d, dtype=torch.bfloat16, seed=0):
  """A pool of shuffled pages: P / page shared prefix pages in every row of the table, then each sequence's own pages (suffix[b] keys)."""
  g = torch.Generator().manual_seed(seed)
  npre = P // page
  own = [max(1, -(-s // page)) for s in suffix]
  ppr = npre + max(own)
  n_pages = npre + sum(own)
  ids = torch.randperm(n_pages, generator=g).to(torch.int32)
  table = torch.empty((B, ppr), dtype=torch.int32)
  table[:, :npre] = ids[:npre]
  nxt = npre
  for b in range(B):
    table[b, npre:npre + own[b]] = ids[nxt:nxt + own[b]]
    table[b, npre + own[b]:] = ids[nxt + own[b] - 1]  # (unused entries: a valid page of the sequence's own)
    nxt += own[b]
  pk = torch.randn((n_pages, page, hkv, d), dtype=dtype, device="cuda")
  pv = torch.randn((n_pages, page, hkv, d), dtype=dtype, device="cuda")
  lens = torch.tensor([P + s for s in suffix], dtype=torch.int32, device="cuda")
  return pk, pv, table.cuda(), lens


def _time(fn, iters):
  s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  s.record()
  for _ in range(iters):
    fn()
  e.record()
  torch.cuda.synchronize()
  return s.elapsed_time(e) * 1e3 / iters  # us


def _graph(fn):
  fn()
  torch.cuda.synchronize()
  g = torch.cuda.CUDAGraph()
  s = torch.cuda.Stream()
  s.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(s):
    fn()
  torch.cuda.current_stream().wait_stream(s)
  with torch.cuda.graph(g):
    fn()
  torch.cuda.synchronize()
  return g.replay


def run(B, sq, hq, hkv, d, P, page, rounds, iters, eager=True, seed=0, tag="grid"):
  gen = torch.Generator().manual_seed(seed + B * 7 + P)
  suffix = [int(x) for x in torch.randint(128, 2049, (B,), generator=gen)]
  pk, pv, table, lens = shared_case(B, P, suffix, page, hkv, d, seed=seed)
  q = torch.randn((B, sq, hq, d), dtype=torch.bfloat16, device="cuda")

  def call(mode):
    return lambda: ffpa_attn_with_kvcache_cascade(q, pk, pv, cache_seqlens=lens, block_table=table, shared_prefix_len=P, causal=True, cascade=mode)

  ref = call(False)()
  got = call(True)()
  err = (got.float() - ref.float()).abs().max().item()
  fns = {"plain": _graph(call(False)), "cascade": _graph(call(True))}
  if eager:
    fns["plain eager"] = call(False)
    fns["cascade eager"] = call(True)
  for fn in fns.values():
    fn()
  torch.cuda.synchronize()
  times = {k: [] for k in fns}
  for _ in range(rounds):
    for k, fn in fns.items():
      times[k].append(_time(fn, iters))
  med = {k: statistics.median(v) for k, v in times.items()}
  prefix_mib = 2 * P * hkv * d * 2 / 2 ** 20
  row = {"set": tag, "B": B, "Sq": sq, "Hq": hq, "Hkv": hkv, "D": d, "P": P, "page": page, "suffix_mean": round(sum(suffix) / B), "prefix_kv_MiB": prefix_mib,
         "us": {k: round(v, 2) for k, v in med.items()}, "cascade_speedup": round(med["plain"] / med["cascade"], 3),
         "max_abs_diff_vs_plain": err}
  if eager:
    row["cascade_speedup_eager"] = round(med["plain eager"] / med["cascade eager"], 3)
  print(json.dumps(row), flush=True)
  del pk, pv
  torch.cuda.empty_cache()
  return row


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--rounds", type=int, default=7)
  ap.add_argument("--iters", type=int, default=20)
  ap.add_argument("--quick", action="store_true", help="one shape per head dim, 1 round of 5 (for the rocprofv3 kernel-trace run)")
  ap.add_argument("--check", action="store_true", help="the check rows (page 256; GQA group 8) instead of the grid")
  ap.add_argument("--dims", default="512,1024")
  ap.add_argument("--out", default=None)
  args = ap.parse_args()
  heads = {512: (32, 8), 1024: (16, 4)}
  rows = []
  if args.check:
    for hq, hkv, page in ((32, 8, 256), (64, 8, 64)):
      for B, sq, P in ((16, 1, 8192), (4, 1, 32768), (64, 4, 2048), (16, 4, 2048), (4, 1, 8192)):
        rows.append(run(B, sq, hq, hkv, 512, P, page, args.rounds, args.iters, tag="check"))
  for d in ([] if args.check else [int(x) for x in args.dims.split(",")]):
    hq, hkv = heads[d]
    if args.quick:
      rows.append(run(16, 1, hq, hkv, d, 8192, 64, 1, 5, eager=False))
      continue
    for P in (2048, 8192, 32768):
      for B in (4, 16, 64):
        for sq in (1, 4):
          rows.append(run(B, sq, hq, hkv, d, P, 64, args.rounds, args.iters))
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
      json.dump({"device": torch.cuda.get_device_name(0), "method": "interleaved rounds, median of per-round means; graph replay (eager: Python launches)",
                 "rows": rows}, f, indent=1)


if __name__ == "__main__":
  main()
