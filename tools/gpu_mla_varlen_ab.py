"""Developer tool: what the ragged MLA latent-cache call costs on the steps of a continuous-batching engine, and whether its compact grid pays
(profiles/r18_mla_varlen.md).

  python tools/gpu_mla_varlen_ab.py [--out profiles/r18_mla_varlen.json] [--rounds 5] [--iters 20] [--only NAME]
        per batch, arms on the SAME tensors, interleaved, warmed, by graph replay (attention only: every arm reads the cache as it is):
          (ragged)  ffpa_attn_varlen_with_kvcache_mla with its own plan;
          (ragged2) the same arm again, as an arm of its own in the same rounds: ragged2 / ragged is the run-to-run spread every ratio is read against;
          (full)    the ragged call with FFPA_FLAG_NO_COMPACT_GRID: the grid that max_seqlen_q sizes;
          (padded)  ffpa_attn_with_kvcache_mla on q padded to the longest sequence (skipped above --max-padded-rows query rows);
          (per_len) one ffpa_attn_with_kvcache_mla call per distinct query length, all in one graph;
          (append)  the ragged append launch alone (ffpa_attn::_mla_append_varlen_hip on the step's new rows).
        and, on uniform decode batches (32 x 1 token), the ragged call against ffpa_attn_with_kvcache_mla: the same kernel and plan, only the host path differs
        (under graph replay: nothing; launched eagerly: the Python in front of the launch).

Batches: 32 sequences whose query lengths cycle 1 - 4 (MTP verification); 63 decodes + one 64-token chunk; 63 decodes + one 512-token chunk; 28 decodes + four
11-token verifications (the batch that sits exactly on the compact rule's threshold at Hq 128); each at Hq 16 and
Hq 128 on one latent head, 4k and 16k keys per sequence, causal.  D = 576, head_dim_v = 512, bf16, pages of 64 keys, scale 1 / sqrt(192).  Every figure is the
median of `--rounds` interleaved rounds of up to `--iters` replays each (fewer for arms that take long: a round of an arm is held near 40 ms), timed with
device events."""

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PAGE, D, DV = 64, 576, 512
SCALE = 192 ** -0.5
BATCHES = {
  "mtp": [1 + i % 4 for i in range(32)],
  "chunk64": [1] * 63 + [64],
  "chunk512": [1] * 63 + [512],
  "edge": [1] * 28 + [11] * 4,  # exactly at the compact rule's threshold at Hq 128: 4 x 176 slots = 32 x 22 row tiles (three quarters of the full grid idle)
}
UNIFORM = [1] * 32


def graphed(fn):
  side = torch.cuda.Stream()
  side.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(side):
    for _ in range(2):
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
  n = {}
  for k, run in arms.items():  # warm-up, and how many replays keep a round of this arm near 40 ms
    n[k] = max(1, min(iters, int(40000.0 / max(time_us(run, 1), 1.0))))
  samples = {k: [] for k in arms}
  for _ in range(rounds):
    for k, run in arms.items():
      samples[k].append(time_us(run, n[k]))
  return {k: (statistics.median(v), min(v), max(v)) for k, v in samples.items()}


def with_flags(hip, flags, plan, fn):
  """``fn()`` with ``flags`` on every MLA launch inside it and the launch's plan in ``plan``."""
  real = hip.mla_forward

  def spy(*a, **kw):
    kw["flags"] = kw.get("flags", 0) | flags
    kw["plan_out"] = plan
    return real(*a, **kw)

  hip.mla_forward = spy
  try:
    return fn()
  finally:
    hip.mla_forward = real


def brief(p):
  return (f"{p['workgroups']} wg, {p['row_tiles']} row tiles, {p['splits']} splits{', compact ' + str(p['compact_slots']) if p.get('compact_slots') else ''}"
          f"{', NT' if ', NT>' in p['kernel'] else ''}")


def run_batch(name, qlens, hq, L, args, hip):
  from ffpa_attn_amd import ffpa_attn_varlen_with_kvcache_mla, ffpa_attn_with_kvcache_mla

  g = torch.Generator(device="cuda").manual_seed(0)
  B, T, max_q = len(qlens), sum(qlens), max(qlens)
  pps = L // PAGE + -(-max_q // PAGE)  # (room for the step's own rows: the append arm writes them behind the L keys)
  pool = torch.randn((B * pps, PAGE, 1, D), generator=g, device="cuda", dtype=torch.bfloat16)
  table = torch.randperm(B * pps, device="cuda", generator=g).to(torch.int32).view(B, pps)
  q = torch.randn((T, hq, D), generator=g, device="cuda", dtype=torch.bfloat16)
  kv_new = torch.randn((T, 1, D), generator=g, device="cuda", dtype=torch.bfloat16)
  cu = torch.tensor([0] + [sum(qlens[:i + 1]) for i in range(B)], dtype=torch.int32, device="cuda")
  lens = torch.full((B,), L, dtype=torch.int32, device="cuda")
  ragged = lambda: ffpa_attn_varlen_with_kvcache_mla(q, pool, DV, cu, max_q, lens, table, softmax_scale=SCALE, causal=True)
  plans = {"ragged": {}, "full": {}}
  want = with_flags(hip, 0, plans["ragged"], ragged)
  full_out = with_flags(hip, hip.FLAG_NO_COMPACT_GRID, plans["full"], ragged)
  if plans["ragged"]["splits"] == plans["full"]["splits"]:
    assert torch.equal(want, full_out), "the full grid and the compact grid differ"
  else:  # (the split rule runs on the grid that is launched: another count of KV ranges, another rounding in the merge)
    torch.testing.assert_close(want.float(), full_out.float(), atol=2e-2, rtol=2e-2)
  arms = {"ragged": graphed(ragged), "ragged2": graphed(ragged)}
  arms["full"] = with_flags(hip, hip.FLAG_NO_COMPACT_GRID, {}, lambda: graphed(ragged))
  # one uniform call per distinct length, on tensors gathered beforehand
  groups = []
  starts = cu.tolist()
  for n in sorted(set(qlens)):
    idx = [b for b in range(B) if qlens[b] == n]
    qn = torch.stack([q[starts[b]:starts[b] + n] for b in idx])
    groups.append((qn, table[idx].contiguous(), lens[idx].contiguous(), idx, n))
  per_len = lambda: [ffpa_attn_with_kvcache_mla(qn, pool, DV, cache_seqlens=ln, block_table=tn, softmax_scale=SCALE, causal=True) for qn, tn, ln, _, _ in groups]
  for o, (_, _, _, idx, n) in zip(per_len(), groups):
    for j, b in enumerate(idx):
      torch.testing.assert_close(o[j].float(), want[starts[b]:starts[b] + n].float(), atol=2e-2, rtol=2e-2)  # (the routes compute the same thing)
  arms["per_len"] = graphed(per_len)
  padded_rows = B * max_q * hq
  if len(set(qlens)) > 1 and padded_rows <= args.max_padded_rows:
    qp = torch.zeros((B, max_q, hq, D), device="cuda", dtype=torch.bfloat16)
    for b in range(B):
      qp[b, max_q - qlens[b]:] = q[starts[b]:starts[b + 1]]  # (bottom-right aligned: the last tokens are the sequence's own)
    arms["padded"] = graphed(lambda: ffpa_attn_with_kvcache_mla(qp, pool, DV, cache_seqlens=lens, block_table=table, softmax_scale=SCALE, causal=True))
  arms["append"] = graphed(lambda: torch.ops.ffpa_attn._mla_append_varlen_hip(pool, kv_new, cu, lens, table))
  if len(set(qlens)) == 1:
    qu = q.view(B, max_q, hq, D)
    uniform = lambda: ffpa_attn_with_kvcache_mla(qu, pool, DV, cache_seqlens=lens, block_table=table, softmax_scale=SCALE, causal=max_q > 1)
    assert torch.equal(uniform().view(T, hq, DV), want)
    arms["uniform"] = graphed(uniform)
  r = interleaved(arms, args.rounds, args.iters)
  rec = {"batch": name, "B": B, "tokens": T, "max_q": max_q, "Hq": hq, "L": L, "plan_ragged": brief(plans["ragged"]), "plan_full": brief(plans["full"]),
         "compact_taken": bool(plans["ragged"].get("compact_slots"))}
  for k, v in r.items():
    rec[k + "_us"] = round(v[0], 2)
    rec[k + "_min_max"] = [round(x, 2) for x in v[1:]]
  rec["spread"] = round(r["ragged2"][0] / r["ragged"][0], 4)
  for k in ("full", "padded", "per_len", "uniform"):
    if k in r:
      rec[k + "_over_ragged"] = round(r[k][0] / r["ragged"][0], 3)
  if "padded" not in arms and len(set(qlens)) > 1:
    rec["padded_us"] = f"not run ({padded_rows} padded query rows)"
  if "uniform" in arms:
    # launched eagerly: the host path in front of the same launches (wall clock per call over a synchronised loop)
    import time
    for k, fn in (("ragged", ragged), ("uniform", uniform)):
      fn()
      torch.cuda.synchronize()
      t0 = time.perf_counter()
      for _ in range(200):
        fn()
      torch.cuda.synchronize()
      rec[k + "_eager_us"] = round((time.perf_counter() - t0) / 200 * 1e6, 2)
  return rec


def write_md(path, records):
  cols = ["batch", "Hq", "L", "tokens", "ragged_us", "spread", "full_us", "full_over_ragged", "padded_us", "padded_over_ragged", "per_len_us", "per_len_over_ragged",
          "append_us", "uniform_us", "uniform_over_ragged", "ragged_eager_us", "uniform_eager_us", "plan_ragged", "plan_full"]
  rows = ["| " + " | ".join(cols) + " |", "|" + "---|" * len(cols)]
  for r in records:
    rows.append("| " + " | ".join(str(r.get(c, "")) for c in cols) + " |")
  with open(path, "w") as f:
    f.write("\n".join(rows) + "\n")


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--rounds", type=int, default=5)
  ap.add_argument("--iters", type=int, default=20)
  ap.add_argument("--only", default=None, help="one batch name (mtp, chunk64, chunk512, edge, uniform)")
  ap.add_argument("--keys", type=lambda s: [int(x) for x in s.split(",")], default=[4096, 16384])
  ap.add_argument("--max-padded-rows", type=int, default=1 << 20)
  ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r18_mla_varlen.json"))
  args = ap.parse_args()
  from ffpa_attn_amd import hip

  assert torch.cuda.is_available(), "needs a GPU"
  records = []
  for name, qlens in list(BATCHES.items()) + [("uniform", UNIFORM)]:
    if args.only and name != args.only:
      continue
    for hq in (16, 128):
      for L in args.keys:
        rec = run_batch(name, qlens, hq, L, args, hip)
        records.append(rec)
        print(json.dumps(rec), flush=True)
        torch.cuda.empty_cache()
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, "w") as f:
    json.dump({"tool": "tools/gpu_mla_varlen_ab.py", "rounds": args.rounds, "iters": args.iters, "records": records}, f, indent=1)
  write_md(os.path.splitext(args.out)[0] + "_table.md", records)


if __name__ == "__main__":
  main()
