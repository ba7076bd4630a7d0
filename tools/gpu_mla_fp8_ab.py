"""Developer tool: the FP8 latent-cache call against the 16-bit latent call on the dequantised tensors (profiles/r22_mla_fp8.md).  A measurement, not a gate.

  python tools/gpu_mla_fp8_ab.py [--out profiles/r22_mla_fp8.json] [--rounds 7] [--iters 20]
        arms per shape on the same q, table and lengths, interleaved, warmed, by graph replay:
          (fp8)   ffpa_attn_with_kvcache_mla_fp8(q, pool8, 512, kv_scale=0.5, ...): the pool holds OCP e4m3 codes, one byte per element;
          (bf16)  ffpa_attn_with_kvcache_mla(q, pool8.to(bf16), 512, softmax_scale * 0.5, ...): the 16-bit latent call on the dequantised pool;
          (bf16b) arm (bf16) again, as an arm of its own in the same rounds: bf16b / bf16 is the run-to-run spread the ratio is read against;
        and the two appends of one new row per sequence, each with its attention launch (the append has no graph of its own: the call captures both):
          (fp8+kv) / (bf16+kv) the same calls with kv=: the difference to the arm without kv is what the quantising / the copying append costs.
        Writes the records as JSON and a markdown table next to it.

Shapes (profiles/r16_mla.md's): B 32, pages of 64 keys, 1k / 4k / 16k keys per sequence, Hq 16 and Hq 128 on one latent head at one token, Hq 16 at four tokens
causal.  D = 576, head_dim_v = 512, bf16 q, scale 1 / sqrt(192).  Bytes are ALGORITHMIC — B x L x 576 B for the FP8 pool, twice that for the bf16 pool — and the
TB/s divide them by the median time.  Every figure is the median of `--rounds` interleaved rounds of `--iters` replays each, timed with device events."""

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

B, PAGE, D, DV = 32, 64, 576, 512
SCALE = 192 ** -0.5
KV_SCALE = 0.5
SHAPES = [(hq, 1, L) for hq in (16, 128) for L in (1024, 4096, 16384)] + [(16, 4, L) for L in (1024, 4096, 16384)]  # (Hq, tokens, keys)


def batch(hq, sq, L, seed=0):
  from ffpa_attn_amd import quantize_latent_rows

  g = torch.Generator(device="cuda").manual_seed(seed)
  pps = L // PAGE + 1  # (one page of room: the append arms write one row per sequence)
  n_pages = B * pps
  pool8 = quantize_latent_rows(torch.randn((n_pages, PAGE, 1, D), generator=g, device="cuda", dtype=torch.bfloat16), KV_SCALE)
  table = torch.randperm(n_pages, device="cuda", generator=g).to(torch.int32).view(B, pps)
  q = torch.randn((B, sq, hq, D), generator=g, device="cuda", dtype=torch.bfloat16)
  kv = torch.randn((B, 1, 1, D), generator=g, device="cuda", dtype=torch.bfloat16)
  return q, pool8, table, kv


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
  rows = ["| Hq | tokens | keys | fp8 us | bf16 us | bf16 / fp8 | bf16b / bf16 (spread) | fp8 MiB | bf16 MiB | fp8 TB/s | bf16 TB/s | fp8 append us | bf16 append us | plan (fp8) | plan (bf16) |",
          "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
  for r in records:
    rows.append(f"| {r['Hq']} | {r['tokens']} | {r['L']} | {r['fp8_us']} | {r['bf16_us']} | {r['bf16_over_fp8']} | {r['bf16b_over_bf16']} | {r['fp8_mib']} | {r['bf16_mib']} | "
                f"{r['fp8_tbs']} | {r['bf16_tbs']} | {r['fp8_append_us']} | {r['bf16_append_us']} | {r['plan_fp8']} | {r['plan_bf16']} |")
  with open(path, "w") as f:
    f.write("\n".join(rows) + "\n")


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--rounds", type=int, default=7)
  ap.add_argument("--iters", type=int, default=20)
  ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r22_mla_fp8.json"))
  args = ap.parse_args()
  from ffpa_attn_amd import ffpa_attn_with_kvcache_mla, ffpa_attn_with_kvcache_mla_fp8, hip

  assert torch.cuda.is_available(), "needs a GPU"
  records = []
  for hq, sq, L in SHAPES:
    q, pool8, table, kv = batch(hq, sq, L)
    pool16 = pool8.to(torch.bfloat16)
    lens = torch.full((B,), L, dtype=torch.int32, device="cuda")
    causal = sq > 1
    fp8 = lambda rows=None: ffpa_attn_with_kvcache_mla_fp8(q, pool8, DV, kv_scale=KV_SCALE, kv=rows, cache_seqlens=lens, block_table=table, softmax_scale=SCALE,
                                                           causal=causal)
    wide = lambda rows=None: ffpa_attn_with_kvcache_mla(q, pool16, DV, kv=rows, cache_seqlens=lens, block_table=table, softmax_scale=SCALE * KV_SCALE, causal=causal)
    assert torch.equal(fp8(), wide() * KV_SCALE)  # (a power-of-two scale: the two routes return the same bits)
    plans = {"fp8": {}, "bf16": {}}
    real = hip.mla_forward

    def spy(*a, **kw):
      kw["plan_out"] = plans["fp8" if kw.get("kv_scale") is not None else "bf16"]
      return real(*a, **kw)

    hip.mla_forward = spy
    try:
      fp8(), wide()
    finally:
      hip.mla_forward = real
    brief = lambda p: f"{p['workgroups']} wg, {p['row_tiles']} row tiles, {p['splits']} splits{', NT' if ', NT>' in p['kernel'] else ''}{', packed' if 'packed' in p['kernel'] else ''}"
    r = interleaved({"fp8": graphed(fp8), "bf16": graphed(wide), "bf16b": graphed(wide), "fp8+kv": graphed(lambda: fp8(kv)), "bf16+kv": graphed(lambda: wide(kv))},
                    args.rounds, args.iters)
    fp8_bytes, wide_bytes = B * L * D, B * L * D * 2
    rec = {"Hq": hq, "tokens": sq, "B": B, "L": L, "fp8_us": round(r["fp8"][0], 2), "bf16_us": round(r["bf16"][0], 2), "bf16b_us": round(r["bf16b"][0], 2),
           "bf16_over_fp8": round(r["bf16"][0] / r["fp8"][0], 3), "bf16b_over_bf16": round(r["bf16b"][0] / r["bf16"][0], 4),
           "fp8_min_max": [round(x, 2) for x in r["fp8"][1:]], "bf16_min_max": [round(x, 2) for x in r["bf16"][1:]],
           "fp8_mib": round(fp8_bytes / 2 ** 20, 1), "bf16_mib": round(wide_bytes / 2 ** 20, 1),
           "fp8_tbs": round(fp8_bytes / r["fp8"][0] / 1e6, 3), "bf16_tbs": round(wide_bytes / r["bf16"][0] / 1e6, 3),
           "fp8_kv_us": round(r["fp8+kv"][0], 2), "bf16_kv_us": round(r["bf16+kv"][0], 2),
           "fp8_append_us": round(r["fp8+kv"][0] - r["fp8"][0], 2), "bf16_append_us": round(r["bf16+kv"][0] - r["bf16"][0], 2),
           "plan_fp8": brief(plans["fp8"]), "plan_bf16": brief(plans["bf16"])}
    records.append(rec)
    print(json.dumps(rec), flush=True)
    del q, pool8, pool16, table, kv
    torch.cuda.empty_cache()
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, "w") as f:
    json.dump({"tool": "tools/gpu_mla_fp8_ab.py", "rounds": args.rounds, "iters": args.iters, "kv_scale": KV_SCALE, "records": records}, f, indent=1)
  write_md(os.path.splitext(args.out)[0] + "_table.md", records)


if __name__ == "__main__":
  main()
