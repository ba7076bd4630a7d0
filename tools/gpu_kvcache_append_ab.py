"""A/B of a decode step that appends its new keys: ffpa_attn_with_kvcache(k=, v=, rotary_cos=, rotary_sin=) against the torch route a caller writes without it,
interleaved in one process (tools/gpu_paged_ab.py's method: alternating rounds, medians of device-event times).  Rows per workload:

  (a) append+rotary+attend   ffpa_attn_with_kvcache(q, kc, vc, k=, v=, rotary_cos=, rotary_sin=, cache_seqlens=, block_table=): two launches
  (b) torch route            rotary of q and k in torch (fp32), index_put_ of K and V into the pages, the lengths add, then ffpa_attn_with_kvcache without k / v
  (c) attention alone        ffpa_attn_with_kvcache on the already-appended cache (rotated q, post-append lengths): the attention launch of (a)
  (d) append alone           ffpa_attn::_kvcache_append_hip: the prepare launch of (a), back-to-back Python op calls — host-bound, NOT the kernel's time

  python tools/gpu_kvcache_append_ab.py [--rounds 7] [--iters 20] [--out FILE]
  rocprofv3 --kernel-trace --output-format csv -d DIR -o append -- python tools/gpu_kvcache_append_ab.py --rounds 1 --iters 10
  python tools/gpu_kvcache_append_ab.py --from-trace DIR/append_kernel_trace.csv   # the kernels' own times and the append's bandwidth, per workload

Workloads: the varlen_decode batch (32 sequences x 1 token, KV 1k ... 16k, GQA 32 / 8, D 512) paged at 64 and 256 keys per page, and the same batch at D 1024
(page 64); NeoX rotary over the whole head dim, causal (FlashAttention's decode call).  Every call appends at the same positions (cache_seqlens is not advanced),
so each iteration does the same work."""

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from ffpa_attn_amd import ffpa_attn_with_kvcache, hip  # noqa: E402


def _case(lens, snew, page, hkv, d, dtype, seed=0):
  B = len(lens)
  need = [-(-(n + snew) // page) for n in lens]
  ppr = max(need)
  n_pages = sum(need)
  ids = torch.randperm(n_pages, generator=torch.Generator().manual_seed(seed))
  table = torch.zeros((B, ppr), dtype=torch.int32)
  nxt = 0
  for i in range(B):
    table[i, : need[i]] = ids[nxt : nxt + need[i]].to(torch.int32)
    nxt += need[i]
  pk = torch.randn((n_pages, page, hkv, d), dtype=dtype, device="cuda")
  pv = torch.randn((n_pages, page, hkv, d), dtype=dtype, device="cuda")
  return pk, pv, table.cuda(), torch.tensor(lens, dtype=torch.int32, device="cuda")


def _rope(x, cos, sin, pos, rd):
  """NeoX rotary in torch, fp32, one rounding: what a caller writes today"""
  c, s = cos[pos].float()[:, None], sin[pos].float()[:, None]
  x1, x2 = x[..., : rd // 2].float(), x[..., rd // 2 : rd].float()
  return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s, x[..., rd:].float()], -1).to(x.dtype)


WORKLOADS = (("D512 page64", 512, 64), ("D512 page256", 512, 256), ("D1024 page64", 1024, 64))  # (the order main() runs them in)
DECODE = dict(B=32, sq=1, hq=32, snew=1, hkv=8)


def _append_bytes(B, sq, hq, snew, hkv, d):
  """bytes the prepare launch reads + writes: q in / q_rot out, new K / V in and into the cache"""
  return 2 * B * (sq * hq + 2 * snew * hkv) * d * 2


def from_trace(path):
  """Per workload, from a rocprofv3 kernel trace of `--rounds 1 --iters 10`: the append kernel's and the attention kernel's median durations, and the append's
  achieved bandwidth (its bytes over its own kernel time).  The append kernel runs 22 times per workload: warm-up, the output check, 10 x (a), 10 x (d)."""
  import csv

  rows = list(csv.DictReader(open(path)))
  app = [r for r in rows if "ffpa_kv_append_kernel" in r["Kernel_Name"]]
  per = len(app) // len(WORKLOADS)
  print("# rocprofv3 --kernel-trace over `python tools/gpu_kvcache_append_ab.py --rounds 1 --iters 10` on MI355X (the A/B's workloads, in order); durations in us")
  print("workload,kernel,grid_x_threads,grid_y,dispatches,median_us,min_us,max_us,bytes,TBps_at_median")
  for w, (name, d, _) in enumerate(WORKLOADS):
    chunk = app[w * per : (w + 1) * per]
    ds = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in chunk]
    med = statistics.median(ds)
    nbytes = _append_bytes(DECODE["B"], DECODE["sq"], DECODE["hq"], DECODE["snew"], DECODE["hkv"], d)
    print(f"{name},ffpa_kv_append_kernel<bf16, NeoX>,{chunk[0]['Grid_Size_X']},{chunk[0]['Grid_Size_Y']},{len(ds)},{med:.2f},{min(ds):.2f},{max(ds):.2f},"
          f"{nbytes},{nbytes / med / 1e6:.3f}")
  for d in (512, 1024):
    ds = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if "ffpa_fwd_m16_paged_kernel" in r["Kernel_Name"] and f"Li{d}E" in r["Kernel_Name"]]
    print(f"D{d} all pages,ffpa_fwd_m16_paged_kernel<bf16, {d}, NT>,,,{len(ds)},{statistics.median(ds):.2f},{min(ds):.2f},{max(ds):.2f},,")


def _time(fn, iters):
  s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  s.record()
  for _ in range(iters):
    fn()
  e.record()
  torch.cuda.synchronize()
  return s.elapsed_time(e) * 1e3 / iters  # us


def run(name, lens, hq, hkv, d, page, rounds, iters, dtype=torch.bfloat16):
  snew = sq = 1
  B = len(lens)
  pk, pv, table, seqlens = _case(lens, snew, page, hkv, d, dtype)
  cap = table.size(1) * page
  rd = d
  ang = torch.rand((cap, rd // 2), device="cuda") * 6.2831853
  cos, sin = torch.cos(ang).to(dtype), torch.sin(ang).to(dtype)
  q = torch.randn((B, sq, hq, d), dtype=dtype, device="cuda")
  k = torch.randn((B, snew, hkv, d), dtype=dtype, device="cuda")
  v = torch.randn((B, snew, hkv, d), dtype=dtype, device="cuda")
  kw = dict(block_table=table, causal=True)

  def fused():
    return ffpa_attn_with_kvcache(q, pk, pv, k=k, v=v, rotary_cos=cos, rotary_sin=sin, cache_seqlens=seqlens, rotary_interleaved=False, **kw)

  steps = torch.arange(snew, device="cuda")

  def torch_route():
    pos = seqlens.long()[:, None] + steps  # [B, Snew]
    qr = _rope(q.reshape(B * sq, hq, d), cos, sin, (seqlens.long()[:, None] + torch.arange(sq, device="cuda")).flatten(), rd).view_as(q)
    kr = _rope(k.reshape(B * snew, hkv, d), cos, sin, pos.flatten(), rd)
    pid = table.long().gather(1, pos // page).flatten()
    row = (pos % page).flatten()
    pk.index_put_((pid, row), kr)
    pv.index_put_((pid, row), v.reshape(B * snew, hkv, d))
    used = seqlens + snew
    return ffpa_attn_with_kvcache(qr, pk, pv, cache_seqlens=used, **kw)

  q_rot, used = torch.ops.ffpa_attn._kvcache_append_hip(q, pk, pv, k, v, seqlens, table, cos, sin, False, True)

  def attention_alone():
    return ffpa_attn_with_kvcache(q_rot, pk, pv, cache_seqlens=used, **kw)

  def append_alone():
    return torch.ops.ffpa_attn._kvcache_append_hip(q, pk, pv, k, v, seqlens, table, cos, sin, False, True)

  fns = {"(a) append+rotary+attend": fused, "(b) torch route": torch_route, "(c) attention alone": attention_alone, "(d) append alone": append_alone}
  outs = {key: fns[key]() for key in ("(a) append+rotary+attend", "(b) torch route", "(c) attention alone")}
  torch.cuda.synchronize()
  same_ab = bool(torch.equal(outs["(a) append+rotary+attend"], outs["(b) torch route"]))
  same_ac = bool(torch.equal(outs["(a) append+rotary+attend"], outs["(c) attention alone"]))
  times = {key: [] for key in fns}
  for _ in range(rounds):
    for key, fn in fns.items():
      times[key].append(_time(fn, iters))
  med = {key: statistics.median(t) for key, t in times.items()}
  a, b, c = (med[key] for key in list(fns)[:3])
  plan = hip.varlen_launch_plan(B, hq, hkv, sq, max(lens) + snew, d, total_q=B * sq, page_size=page)
  row = {"workload": name, "page": page, "d": d, "rotary_dim": rd, "attention_kernel": plan["kernel"], "us": {key: round(val, 2) for key, val in med.items()},
         "spread_us": {key: [round(min(t), 2), round(max(t), 2)] for key, t in times.items()}, "a_minus_c_us": round(a - c, 2),
         "torch_route_over_fused": round(b / a, 3), "prepare_bytes": _append_bytes(B, sq, hq, snew, hkv, d), "O_a_equals_b": same_ab,
         "O_a_equals_c": same_ac}
  print(json.dumps(row), flush=True)
  return row


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--rounds", type=int, default=7)
  ap.add_argument("--iters", type=int, default=20)
  ap.add_argument("--out", default=None)
  ap.add_argument("--from-trace", default=None, help="print the kernel times of a rocprofv3 kernel trace of this tool instead of timing")
  args = ap.parse_args()
  if args.from_trace:
    from_trace(args.from_trace)
    return
  decode_lens = [1024 + (16384 - 1024) * i // 31 for i in range(DECODE["B"])]
  rows = [run("varlen_decode 32 x 1 token, KV 1k..16k, GQA 32/8", decode_lens, DECODE["hq"], DECODE["hkv"], d, page, args.rounds, args.iters)
          for _, d, page in WORKLOADS]
  if args.out:
    with open(args.out, "w") as f:
      json.dump({"device": torch.cuda.get_device_name(0), "method": "interleaved rounds, median of device-event times per call", "rows": rows}, f, indent=1)


if __name__ == "__main__":
  main()
