"""Developer tool: what the MLA latent-cache call saves on a decode step against the best route there was before it (profiles/r16_mla.md).

  python tools/gpu_mla_ab.py [--out profiles/r16_mla.json] [--rounds 7] [--iters 20]
        two arms per shape on the SAME tensors, interleaved, warmed, by graph replay:
          (new) ffpa_attn_with_kvcache_mla(q, kv, 512, ...): one latent stream, the group's heads packed into rows however many they are;
          (old) ffpa_attn_with_kvcache(q, kv, kv, ...)[..., :512]: the two-cache call on the aliased pool — every latent row is moved twice, 128 heads on one latent
                head run as 128 unpacked workgroups per sequence, and the output carries 64 junk columns (the slice is a view: it costs nothing);
          (old2) arm (old) again, as an arm of its own in the same rounds: old2 / old is the run-to-run spread the ratio is read against.
        Writes the records as JSON and a markdown table next to it.

Shapes: B 32 x 1 token, pages of 64 keys, 1k ... 16k keys per sequence (the bench's varlen_decode family), Hq 16 and Hq 128 on Hkv 1; and B 32 x 4 tokens causal at
Hq 16.  D = 576, head_dim_v = 512, bf16, scale 1 / sqrt(192).  Bytes are ALGORITHMIC: what a route's kernels must move per step if every workgroup's stream came
from memory once per (sequence, KV head) — B x L x 1152 B for the latent call, twice that (K + V) for the two-cache call; the achieved TB/s divide them by the
median time.  Every figure is the median of `--rounds` interleaved rounds of `--iters` replays each, timed with device events."""

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

B, PAGE, D, DV = 32, 64, 576, 512
SCALE = 192 ** -0.5
SHAPES = [(hq, 1, L) for hq in (16, 128) for L in (1024, 4096, 16384)] + [(16, 4, L) for L in (1024, 4096, 16384)]  # (Hq, tokens, keys)


def batch(hq, sq, L, seed=0):
  g = torch.Generator(device="cuda").manual_seed(seed)
  pps = L // PAGE
  n_pages = B * pps
  kv = torch.randn((n_pages, PAGE, 1, D), generator=g, device="cuda", dtype=torch.bfloat16)
  table = torch.randperm(n_pages, device="cuda", generator=g).to(torch.int32).view(B, pps)
  q = torch.randn((B, sq, hq, D), generator=g, device="cuda", dtype=torch.bfloat16)
  return q, kv, table


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
  rows = ["| Hq | tokens | keys | new us | old us | old / new | old2 / old (spread) | new bytes (MiB) | old bytes (MiB) | new TB/s | old TB/s | plan (new) | plan (old) |",
          "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
  for r in records:
    rows.append(f"| {r['Hq']} | {r['tokens']} | {r['L']} | {r['new_us']} | {r['old_us']} | {r['old_over_new']} | {r['old2_over_old']} | {r['new_mib']} | {r['old_mib']} | "
                f"{r['new_tbs']} | {r['old_tbs']} | {r['plan_new']} | {r['plan_old']} |")
  with open(path, "w") as f:
    f.write("\n".join(rows) + "\n")


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--rounds", type=int, default=7)
  ap.add_argument("--iters", type=int, default=20)
  ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r16_mla.json"))
  args = ap.parse_args()
  from ffpa_attn_amd import ffpa_attn_with_kvcache, ffpa_attn_with_kvcache_mla, hip

  assert torch.cuda.is_available(), "needs a GPU"
  records = []
  for hq, sq, L in SHAPES:
    q, kv, table = batch(hq, sq, L)
    lens = torch.full((B,), L, dtype=torch.int32, device="cuda")
    causal = sq > 1
    new = lambda: ffpa_attn_with_kvcache_mla(q, kv, DV, cache_seqlens=lens, block_table=table, softmax_scale=SCALE, causal=causal)
    old = lambda: ffpa_attn_with_kvcache(q, kv, kv, cache_seqlens=lens, block_table=table, softmax_scale=SCALE, causal=causal)[..., :DV]
    torch.testing.assert_close(new().float(), old().float(), atol=2e-2, rtol=2e-2)  # (the two routes compute the same thing)
    plans = {}
    real_mla, real_var = hip.mla_forward, hip.varlen_forward
    for key, real, name in (("new", real_mla, "mla_forward"), ("old", real_var, "varlen_forward")):
      def spy(*a, _real=real, _key=key, **kw):
        kw["plan_out"] = plans.setdefault(_key, {})
        return _real(*a, **kw)
      setattr(hip, name, spy)
    try:
      new(), old()
    finally:
      hip.mla_forward, hip.varlen_forward = real_mla, real_var
    brief = lambda p: f"{p['workgroups']} wg, {p['row_tiles']} row tiles, {p['splits']} splits{', NT' if ', NT>' in p['kernel'] else ''}{', packed' if 'packed' in p['kernel'] else ''}"
    r = interleaved({"new": graphed(new), "old": graphed(old), "old2": graphed(old)}, args.rounds, args.iters)
    new_bytes, old_bytes = B * L * D * 2, 2 * B * L * D * 2
    rec = {"Hq": hq, "tokens": sq, "B": B, "L": L, "new_us": round(r["new"][0], 2), "old_us": round(r["old"][0], 2), "old2_us": round(r["old2"][0], 2),
           "old_over_new": round(r["old"][0] / r["new"][0], 3), "old2_over_old": round(r["old2"][0] / r["old"][0], 4),
           "new_min_max": [round(x, 2) for x in r["new"][1:]], "old_min_max": [round(x, 2) for x in r["old"][1:]],
           "new_mib": round(new_bytes / 2 ** 20, 1), "old_mib": round(old_bytes / 2 ** 20, 1),
           "new_tbs": round(new_bytes / r["new"][0] / 1e6, 3), "old_tbs": round(old_bytes / r["old"][0] / 1e6, 3),
           "plan_new": brief(plans["new"]), "plan_old": brief(plans["old"])}
    records.append(rec)
    print(json.dumps(rec), flush=True)
    del q, kv, table
    torch.cuda.empty_cache()
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, "w") as f:
    json.dump({"tool": "tools/gpu_mla_ab.py", "rounds": args.rounds, "iters": args.iters, "records": records}, f, indent=1)
  write_md(os.path.splitext(args.out)[0] + "_table.md", records)


if __name__ == "__main__":
  main()
