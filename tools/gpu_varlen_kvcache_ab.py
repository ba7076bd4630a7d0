"""A/B of a RAGGED step over the paged KV cache: ffpa_attn_varlen_with_kvcache against what a caller does without it, interleaved in one process
(tools/gpu_kvcache_append_ab.py's method: alternating rounds, medians of device-event times), each row timed launched eagerly AND as the replay of one HIP graph.

  uniform decode   the varlen_decode batch (32 sequences x 1 token, KV 1k ... 16k, page 64, NeoX rotary over the whole head dim, causal):
    (a) ragged call      ffpa_attn_varlen_with_kvcache, cu_seqlens_q = arange
    (b) uniform call     ffpa_attn_with_kvcache on the same tensors — the same attention launch: the difference is the two append kernels and the host side
  mixed step       1 x 512-token prompt chunk against 8k keys + 31 decodes at 1k ... 16k, as one batch of 543 token rows:
    (a) ragged call      one ffpa_attn_varlen_with_kvcache
    (b) two calls        ffpa_attn_with_kvcache for the chunk (B 1, Sq 512) and for the decodes (B 31, Sq 1): what a caller does today
    (c) padded call      ffpa_attn_with_kvcache with every sequence padded to Sq 512 (B 32 x 512 rows; the pad rows append garbage behind the decodes' keys:
                         timing only)
    (d) torch append     rotary in torch (fp32), index_put_ of K and V by a slot mapping, the lengths add, then the ragged call without k / v

  python tools/gpu_varlen_kvcache_ab.py [--rounds 7] [--iters 20] [--only decode|mixed] [--dims 512,1024] [--out FILE]
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o varlen -- python tools/gpu_varlen_kvcache_ab.py --only decode --rounds 1 --iters 10 --no-graph
  python tools/gpu_varlen_kvcache_ab.py --from-trace DIR/.../varlen_kernel_trace.csv   # the two append kernels' own times

D 512 runs GQA 32 / 8, D 1024 GQA 16 / 4.  No call advances cache_seqlens, so each iteration does the same work."""

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from ffpa_attn_amd import ffpa_attn_varlen_with_kvcache, ffpa_attn_with_kvcache  # noqa: E402

PAGE = 64
HEADS = {512: (32, 8), 1024: (16, 4)}
DECODE_LENS = [1024 + (16384 - 1024) * i // 31 for i in range(32)]


def _pool(lens, room, hkv, d, dtype, seed=0):
  """Shuffled pages for sequences of ``lens`` keys with ``room`` more to append -> (k pool, v pool, table, lens on the device)."""
  need = [-(-(n + room) // PAGE) for n in lens]
  ids = torch.randperm(sum(need), generator=torch.Generator().manual_seed(seed)).to(torch.int32)
  table = torch.zeros((len(lens), max(need)), dtype=torch.int32)
  nxt = 0
  for i, n in enumerate(need):
    table[i, :n] = ids[nxt:nxt + n]
    nxt += n
  pk = torch.randn((sum(need), PAGE, hkv, d), dtype=dtype, device="cuda")
  pv = torch.randn((sum(need), PAGE, hkv, d), dtype=dtype, device="cuda")
  return pk, pv, table.cuda(), torch.tensor(lens, dtype=torch.int32, device="cuda")


def _rope(x, cos, sin, pos, rd):
  """NeoX rotary in torch, fp32, one rounding: what a caller writes today"""
  c, s = cos[pos].float()[:, None], sin[pos].float()[:, None]
  x1, x2 = x[..., : rd // 2].float(), x[..., rd // 2 : rd].float()
  return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s, x[..., rd:].float()], -1).to(x.dtype)


def _time(fn, iters):
  s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  s.record()
  for _ in range(iters):
    fn()
  e.record()
  torch.cuda.synchronize()
  return s.elapsed_time(e) * 1e3 / iters  # us


def _graphed(fn):
  """``fn`` captured into one HIP graph (after a warm-up on a side stream) -> its replay."""
  side = torch.cuda.Stream()
  side.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(side):
    fn()
  torch.cuda.current_stream().wait_stream(side)
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    fn()
  return graph.replay


def _ab(name, d, fns, rounds, iters, graph, extra):
  modes = {"eager": fns}
  if graph:
    modes["graph"] = {key: _graphed(fn) for key, fn in fns.items()}
  row = {"workload": name, "d": d, "heads": list(HEADS[d]), "page": PAGE, **extra}
  for mode, table in modes.items():
    times = {key: [] for key in table}
    for _ in range(rounds):
      for key, fn in table.items():
        times[key].append(_time(fn, iters))
    med = {key: statistics.median(t) for key, t in times.items()}
    first = next(iter(med))
    row[mode] = {"us": {key: round(val, 2) for key, val in med.items()}, "spread_us": {key: [round(min(t), 2), round(max(t), 2)] for key, t in times.items()},
                 "over_ragged": {key: round(val / med[first], 3) for key, val in med.items()}}
  print(json.dumps(row), flush=True)
  return row


def decode(d, rounds, iters, graph, dtype=torch.bfloat16):
  hq, hkv = HEADS[d]
  B = len(DECODE_LENS)
  pk, pv, table, lens = _pool(DECODE_LENS, 1, hkv, d, dtype)
  cap = table.size(1) * PAGE
  ang = torch.rand((cap, d // 2), device="cuda") * 6.2831853
  cos, sin = torch.cos(ang).to(dtype), torch.sin(ang).to(dtype)
  q, k, v = (torch.randn((B, h, d), dtype=dtype, device="cuda") for h in (hq, hkv, hkv))
  cu = torch.arange(B + 1, dtype=torch.int32, device="cuda")
  kw = dict(rotary_cos=cos, rotary_sin=sin, causal=True, rotary_interleaved=False)
  ragged = lambda: ffpa_attn_varlen_with_kvcache(q, pk, pv, cu, 1, lens, table, k=k, v=v, **kw)
  uniform = lambda: ffpa_attn_with_kvcache(q[:, None], pk, pv, k=k[:, None], v=v[:, None], cache_seqlens=lens, block_table=table, **kw)
  same = bool(torch.equal(ragged(), uniform()[:, 0]))
  return _ab("uniform decode 32 x 1 token, KV 1k..16k", d, {"(a) ragged call": ragged, "(b) uniform call": uniform}, rounds, iters, graph, {"O_a_equals_b": same})


def mixed(d, rounds, iters, graph, dtype=torch.bfloat16):
  hq, hkv = HEADS[d]
  chunk = 512
  seqs = [chunk] + [1] * 31
  lens_l = [8192] + DECODE_LENS[1:]
  B, T = len(seqs), sum(seqs)
  pk, pv, table, lens = _pool(lens_l, chunk, hkv, d, dtype)  # (room for the padded call's 512 rows behind every sequence)
  cap = table.size(1) * PAGE
  ang = torch.rand((cap, d // 2), device="cuda") * 6.2831853
  cos, sin = torch.cos(ang).to(dtype), torch.sin(ang).to(dtype)
  q, k, v = (torch.randn((T, h, d), dtype=dtype, device="cuda") for h in (hq, hkv, hkv))
  cu = torch.tensor([0] + [sum(seqs[:i + 1]) for i in range(B)], dtype=torch.int32, device="cuda")
  kw = dict(rotary_cos=cos, rotary_sin=sin, causal=True, rotary_interleaved=False)
  ragged = lambda: ffpa_attn_varlen_with_kvcache(q, pk, pv, cu, chunk, lens, table, k=k, v=v, **kw)

  def two_calls():
    o1 = ffpa_attn_with_kvcache(q[None, :chunk], pk, pv, k=k[None, :chunk], v=v[None, :chunk], cache_seqlens=lens[:1], block_table=table[:1], **kw)
    o2 = ffpa_attn_with_kvcache(q[chunk:, None], pk, pv, k=k[chunk:, None], v=v[chunk:, None], cache_seqlens=lens[1:], block_table=table[1:], **kw)
    return o1, o2

  qp, kp, vp = (torch.randn((B, chunk, h, d), dtype=dtype, device="cuda") for h in (hq, hkv, hkv))
  padded = lambda: ffpa_attn_with_kvcache(qp, pk, pv, k=kp, v=vp, cache_seqlens=lens, block_table=table, **kw)

  owner = torch.repeat_interleave(torch.arange(B, device="cuda"), torch.tensor(seqs, device="cuda"))
  index = torch.arange(T, device="cuda") - cu.long()[owner]

  def torch_append():
    pos = lens.long()[owner] + index  # the slot mapping of the step, made on the device
    qr, kr = _rope(q, cos, sin, pos, d), _rope(k, cos, sin, pos, d)
    pid = table.long()[owner, pos // PAGE]
    pk.index_put_((pid, pos % PAGE), kr)
    pv.index_put_((pid, pos % PAGE), v)
    used = lens + (cu[1:] - cu[:-1])
    return ffpa_attn_varlen_with_kvcache(qr, pk, pv, cu, chunk, used, table, causal=True)

  o_a, (o1, o2) = ragged(), two_calls()
  same = bool(torch.equal(o_a[:chunk], o1[0]) and torch.equal(o_a[chunk:], o2[:, 0]))
  fns = {"(a) ragged call": ragged, "(b) two uniform calls": two_calls, "(c) padded uniform call": padded, "(d) torch append + ragged attention": torch_append}
  return _ab("mixed step: 1 x 512-token chunk at 8k + 31 decodes at 1k..16k", d, fns, rounds, iters, graph, {"O_a_equals_b": same, "token_rows": T})


def from_trace(path):
  """The append kernels' own times from a rocprofv3 kernel trace of ``--only decode --no-graph``: median / min / max duration per kernel and head dim."""
  import csv

  rows = list(csv.DictReader(open(path)))
  print("kernel,dispatches,median_us,min_us,max_us")
  for name in ("ffpa_kv_append_varlen_kernel", "ffpa_kv_append_kernel"):
    ds = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if name + "I" in r["Kernel_Name"] or name + "<" in r["Kernel_Name"]]
    if ds:
      print(f"{name},{len(ds)},{statistics.median(ds):.2f},{min(ds):.2f},{max(ds):.2f}")


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--rounds", type=int, default=7)
  ap.add_argument("--iters", type=int, default=20)
  ap.add_argument("--only", choices=("decode", "mixed"), default=None)
  ap.add_argument("--dims", type=lambda s: [int(x) for x in s.split(",")], default=[512, 1024])
  ap.add_argument("--no-graph", action="store_true")
  ap.add_argument("--out", default=None)
  ap.add_argument("--from-trace", default=None, help="print the append kernels' times of a rocprofv3 kernel trace of this tool instead of timing")
  args = ap.parse_args()
  if args.from_trace:
    from_trace(args.from_trace)
    return
  rows = []
  for d in args.dims:
    if args.only in (None, "decode"):
      rows.append(decode(d, args.rounds, args.iters, not args.no_graph))
    if args.only in (None, "mixed"):
      rows.append(mixed(d, args.rounds, args.iters, not args.no_graph))
  if args.out:
    with open(args.out, "w") as f:
      json.dump({"device": torch.cuda.get_device_name(0), "method": "interleaved rounds, median of device-event times per call; eager launches and graph replays",
                 "rounds": args.rounds, "iters": args.iters, "rows": rows}, f, indent=1)


if __name__ == "__main__":
  main()
