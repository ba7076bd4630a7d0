"""A/B of the paged-KV launch against the contiguous seqused_k launch on the same data, interleaved in one process (tools/gpu_ab.py's method: alternating rounds,
medians).  Three rows per workload: the paged launch on a pool of SHUFFLED pages, the contiguous launch on the same keys gathered into [B, capacity, Hkv, D], and
the path a caller has without a paged kernel — gather the pages into a contiguous copy, then the contiguous launch.

  python tools/gpu_paged_ab.py [--rounds 7] [--iters 20] [--pages 64,256] [--out FILE]

Workloads: the varlen_decode batch (32 sequences x 1 token, KV 1k ... 16k, GQA 32 / 8, D 512) and a prefill chunk (8 heads, 512 queries against 8k keys, D 512
and 1024).  At D > 512 the paged launch is also timed with FFPA_FLAG_NO_L2_PREFETCH (the L2 touch of the tile two steps ahead, through the page table, off)."""

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from ffpa_attn_amd import hip  # noqa: E402


def _case(lens, page, hkv, d, dtype=torch.bfloat16, seed=0):
  B = len(lens)
  need = [max(1, -(-n // page)) for n in lens]
  ppr = max(need)
  n_pages = sum(need)
  ids = torch.randperm(n_pages, generator=torch.Generator().manual_seed(seed))
  table = torch.zeros((B, ppr), dtype=torch.int32)
  nxt = 0
  for i in range(B):
    table[i, : need[i]] = ids[nxt : nxt + need[i]].to(torch.int32)
    nxt += need[i]
  table = table.cuda()
  pk = torch.randn((n_pages, page, hkv, d), dtype=dtype, device="cuda")
  pv = torch.randn((n_pages, page, hkv, d), dtype=dtype, device="cuda")
  return pk, pv, table, torch.tensor(lens, dtype=torch.int32, device="cuda")


def _time(fn, iters):
  s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  s.record()
  for _ in range(iters):
    fn()
  e.record()
  torch.cuda.synchronize()
  return s.elapsed_time(e) * 1e3 / iters  # us


def run(name, lens, sq, hq, hkv, d, page, causal, rounds, iters):
  pk, pv, table, used = _case(lens, page, hkv, d)
  B = len(lens)
  cap = table.size(1) * page
  q = torch.randn((B * sq, hq, d), dtype=torch.bfloat16, device="cuda")
  cu_q = torch.arange(0, (B + 1) * sq, sq, dtype=torch.int32, device="cuda")
  cu_k = torch.arange(0, (B + 1) * cap, cap, dtype=torch.int32, device="cuda")
  scale = d ** -0.5
  kc = pk[table.long()].reshape(B * cap, hkv, d)
  vc = pv[table.long()].reshape(B * cap, hkv, d)
  kbuf, vbuf = torch.empty_like(kc), torch.empty_like(vc)
  plan = {}
  hip.varlen_forward(q, pk, pv, cu_q, None, sq, cap, causal, scale, seqused_k=used, block_table=table, plan_out=plan)

  def paged(flags=0):
    return lambda: hip.varlen_forward(q, pk, pv, cu_q, None, sq, cap, causal, scale, seqused_k=used, block_table=table, flags=flags)

  def contig():
    hip.varlen_forward(q, kc, vc, cu_q, cu_k, sq, cap, causal, scale, seqused_k=used)

  def gather_then_contig():
    torch.index_select(pk, 0, table.view(-1), out=kbuf.view(-1, page, hkv, d))
    torch.index_select(pv, 0, table.view(-1), out=vbuf.view(-1, page, hkv, d))
    hip.varlen_forward(q, kbuf, vbuf, cu_q, cu_k, sq, cap, causal, scale, seqused_k=used)

  fns = {"paged": paged(), "contiguous": contig, "gather+contiguous": gather_then_contig}
  if d > 512:
    fns["paged, no L2 touch"] = paged(hip.FLAG_NO_L2_PREFETCH)
  for fn in fns.values():
    fn()
  torch.cuda.synchronize()
  times = {k: [] for k in fns}
  for _ in range(rounds):
    for k, fn in fns.items():
      times[k].append(_time(fn, iters))
  med = {k: statistics.median(v) for k, v in times.items()}
  kv_bytes = 2 * sum(lens) * hkv * d * 2
  row = {"workload": name, "page": page, "d": d, "kernel": plan.get("kernel"), "splits": plan.get("splits"), "us": {k: round(v, 2) for k, v in med.items()},
         "paged_rate_vs_contiguous": round(med["contiguous"] / med["paged"], 4), "gain_vs_gather": round(med["gather+contiguous"] / med["paged"], 3),
         "kv_TBps_paged": round(kv_bytes / med["paged"] / 1e6, 3)}
  print(json.dumps(row), flush=True)
  return row


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--rounds", type=int, default=7)
  ap.add_argument("--iters", type=int, default=20)
  ap.add_argument("--pages", default="64,256")
  ap.add_argument("--out", default=None)
  args = ap.parse_args()
  decode_lens = [1024 + (16384 - 1024) * i // 31 for i in range(32)]
  rows = []
  for page in [int(x) for x in args.pages.split(",")]:
    rows.append(run("varlen_decode 32 x 1 token, KV 1k..16k, GQA 32/8", decode_lens, 1, 32, 8, 512, page, False, args.rounds, args.iters))
    for d in (512, 1024):
      rows.append(run("prefill chunk 8 heads, 512 q x 8k keys", [8192], 512, 8, 8, d, page, True, args.rounds, args.iters))
  if args.out:
    with open(args.out, "w") as f:
      json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)


if __name__ == "__main__":
  main()
