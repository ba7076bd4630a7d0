"""Developer tool: what logit soft-capping costs per launch (profiles/r14_softcap.{json,md}).

  python tools/gpu_softcap_ab.py [--out profiles/r14_softcap.json] [--only decode|chunk]
        three arms per shape, interleaved, warmed, under graph replay, on the same tensors:
          (a)  ffpa_attn_with_kvcache_softcap(softcap=50, window_size=w) — the *_softcap_kernel builds;
          (b)  ffpa_attn_with_kvcache_window(window_size=w)              — the *_window_kernel builds: the same plan, the same tile walk, no cap;
          (b2) arm (b) again, as an arm of its own in the same rounds: b2 / b is the run-to-run spread the ratio a / b is read against.
        Writes the records as JSON and a markdown table next to it.

Shapes: the bench's varlen_decode family — 32 sequences x 1 token, paged (page 64), 32k keys each, GQA 32 / 8 at D 512 and 16 / 4 at D 1024 — with a 4k window
(Gemma 2's local layers) and without one (its global layers), and a 512-token prefill chunk against 8k keys (B 1, causal) at D 512 and D 1024.  Every shape runs
at two scales of q.  x 1: scaled scores ~ N(0, 1), where c tanh(s / c) = s to 1e-3 — both arms see the same scores, the same running-max growth and the same
lazy rescales, so a / b is the price of the cap's instructions alone.  x 32: scores of standard deviation 32, the tanh in its bend — arm (b) then sees raw scores
up to +- 150 whose row max keeps growing (its lazy rescale fires often) where arm (a) sees scores bounded by c: a / b there compares two different softmaxes and
says what a capped layer costs against an uncapped one on such values, not what the tanh costs.  Every figure is the median of `--rounds` interleaved rounds of
`--iters` launches each, timed with device events."""

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PAGE, CAP, Q_FACTORS = 64, 50.0, (1.0, 32.0)
# (name, batch, query tokens, keys per sequence, causal, windows)
FAMILIES = {
  "decode": (32, 1, 32768, False, [(4096, 0), (-1, -1)]),
  "chunk": (1, 512, 8192, True, [(-1, -1)]),
}
SHAPES = [(512, (32, 8)), (1024, (16, 4))]


def batch(B, sq, L, d, heads, seed=0):
  g = torch.Generator(device="cuda").manual_seed(seed)
  hq, hkv = heads
  pps = L // PAGE
  n_pages = B * pps
  kc = torch.randn((n_pages, PAGE, hkv, d), generator=g, device="cuda", dtype=torch.bfloat16)
  vc = torch.randn((n_pages, PAGE, hkv, d), generator=g, device="cuda", dtype=torch.bfloat16)
  table = torch.randperm(n_pages, device="cuda", generator=g).to(torch.int32).view(B, pps)
  q = torch.randn((B, sq, hq, d), generator=g, device="cuda", dtype=torch.bfloat16)
  return q, kc, vc, table


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
  rows = ["| family | D | heads | B x tokens | keys | window | q x | (a) softcap us | (b) window us | a / b | b2 / b (spread) | plan |",
          "|---|---|---|---|---|---|---|---|---|---|---|---|"]
  for r in records:
    rows.append(f"| {r['family']} | {r['D']} | {r['heads'][0]} / {r['heads'][1]} | {r['B']} x {r['Sq']} | {r['L']} | {tuple(r['window'])} | {r['q_factor']:g} | {r['a_us']} | {r['b_us']} | "
                f"{r['a_over_b']} | {r['b2_over_b']} | {r['plan']} |")
  with open(path, "w") as f:
    f.write("\n".join(rows) + "\n")


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--only", choices=sorted(FAMILIES), default=None)
  ap.add_argument("--rounds", type=int, default=7)
  ap.add_argument("--iters", type=int, default=30)
  ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r14_softcap.json"))
  args = ap.parse_args()
  from ffpa_attn_amd import ffpa_attn_with_kvcache_softcap, ffpa_attn_with_kvcache_window, hip

  assert torch.cuda.is_available(), "needs a GPU"
  records = []
  for family, (B, sq, L, causal, windows) in FAMILIES.items():
    if args.only and family != args.only:
      continue
    lens = torch.full((B,), L, dtype=torch.int32, device="cuda")
    for d, heads in SHAPES:
      q1, kc, vc, table = batch(B, sq, L, d, heads)
      for window, factor in ((w, f) for w in windows for f in Q_FACTORS):
        q = q1 * factor
        fa = lambda: ffpa_attn_with_kvcache_softcap(q, kc, vc, cache_seqlens=lens, block_table=table, softcap=CAP, window_size=window, causal=causal)
        fb = lambda: ffpa_attn_with_kvcache_window(q, kc, vc, cache_seqlens=lens, block_table=table, window_size=window, causal=causal)
        plan = hip.varlen_launch_plan(B, heads[0], heads[1], sq, L, d, causal=causal, total_q=B * sq, page_size=PAGE, window=window, softcap=CAP)
        r = interleaved({"a": graphed(fa), "b": graphed(fb), "b2": graphed(fb)}, args.rounds, args.iters)
        rec = {"family": family, "D": d, "heads": list(heads), "B": B, "Sq": sq, "L": L, "causal": causal, "window": list(window), "softcap": CAP, "q_factor": factor, "mode": "graph",
               "a_us": round(r["a"][0], 2), "b_us": round(r["b"][0], 2), "b2_us": round(r["b2"][0], 2), "a_over_b": round(r["a"][0] / r["b"][0], 4),
               "b2_over_b": round(r["b2"][0] / r["b"][0], 4), "a_min_max": [round(x, 2) for x in r["a"][1:]], "b_min_max": [round(x, 2) for x in r["b"][1:]],
               "plan": f"{plan['row_tiles']} row tiles x {plan['block_rows']} rows, {plan['splits']} splits{', NT' if ', NT>' in plan['kernel'] else ''}"}
        records.append(rec)
        print(json.dumps(rec), flush=True)
      del q, q1, kc, vc, table
      torch.cuda.empty_cache()
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, "w") as f:
    json.dump({"tool": "tools/gpu_softcap_ab.py", "rounds": args.rounds, "iters": args.iters, "records": records}, f, indent=1)
  write_md(os.path.splitext(args.out)[0] + "_table.md", records)


if __name__ == "__main__":
  main()
