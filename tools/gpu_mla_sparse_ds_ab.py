"""Developer tool: the sparse latent call over the 656-byte FP8 rows of DeepSeek-V3.2 against its floor, against the route a caller had before it and against the
per-tensor FP8 sparse call, and the store kernel's own time (profiles/r25_mla_sparse_ds.md).  A measurement, not a gate.

  python tools/gpu_mla_sparse_ds_ab.py [--out profiles/r25_mla_sparse_ds.json] [--rounds 7] [--iters 20]
        arms per shape on the same q and indices, interleaved, warmed, by graph replay:
          (A)  the new call on the byte pool;
          (B)  the 16-bit sparse call on the pool unpacked ONCE outside the timed region: the floor (the same image, fetched by LDS-DMA);
          (B') arm (B) again, as an arm of its own in the same rounds: B' / B is the run-to-run spread every ratio is read against;
          (C)  the route a caller has without the new call, all of it inside the graph: unpack the step's T x topk selected rows into a 16-bit scratch pool, then
               the 16-bit sparse call with identity indices;
          (D)  the per-tensor FP8 sparse call on a pool of as many rows (576 bytes per row, kv_scale 0.5);
          (S)  the store kernel alone: T rows into T slots.
        Writes the records as JSON and a markdown table next to it.

Shape (profiles/r24_mla_fp8_sparse_tree.md's sparse shape): T = 32 tokens x topk 2048, token t's slots drawn from its own 32k rows of a pool of 32 x 32k rows, Hq 16 /
128, D = 576, head_dim_v = 512, bf16 q, scale 1 / sqrt(192).  Bytes are ALGORITHMIC: rows read x 656 B for the byte pool, x 1152 B for the bf16 pool.  Every figure
is the median of `--rounds` interleaved rounds of `--iters` replays each, timed with device events."""

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gpu_mla_fp8_sparse_tree_ab import graphed, interleaved, plans_of  # noqa: E402

D, DV, ROW = 576, 512, 656
SCALE = 192 ** -0.5
KV_SCALE = 0.5
SHAPES = [(hq, 32, 2048, 32768) for hq in (16, 128)]  # (Hq, tokens, topk, rows per token's sequence)


def records(args):
  from ffpa_attn_amd import (ffpa_attn_with_kvcache_mla_sparse, ffpa_attn_with_kvcache_mla_sparse_ds, ffpa_attn_with_kvcache_mla_sparse_fp8, hip, pack_latent_rows_ds,
                             quantize_latent_rows, store_latent_rows_ds, unpack_latent_rows_ds)

  out = []
  for hq, T, topk, per in SHAPES:
    g = torch.Generator(device="cuda").manual_seed(0)
    rows = T * per
    pool = torch.empty((rows, 1, ROW), dtype=torch.uint8, device="cuda")
    pool16 = torch.empty((rows, 1, D), dtype=torch.bfloat16, device="cuda")
    pool8 = torch.empty((rows, 1, D), dtype=torch.float8_e4m3fn, device="cuda")
    for lo in range(0, rows, 1 << 16):  # (in slabs: the draws of the whole pool need not live at once)
      kv = torch.randn((min(1 << 16, rows - lo), 1, D), generator=g, device="cuda", dtype=torch.bfloat16)
      pool[lo:lo + (1 << 16)] = pack_latent_rows_ds(kv)
      pool16[lo:lo + (1 << 16)] = unpack_latent_rows_ds(pool[lo:lo + (1 << 16)])
      pool8[lo:lo + (1 << 16)] = quantize_latent_rows(kv, KV_SCALE)
    idx = torch.stack([t * per + torch.randperm(per, device="cuda", generator=g)[:topk] for t in range(T)]).to(torch.int32)
    q = torch.randn((T, hq, D), generator=g, device="cuda", dtype=torch.bfloat16)
    scratch = torch.empty((T * topk, 1, D), dtype=torch.bfloat16, device="cuda")
    ident = torch.arange(T * topk, dtype=torch.int32, device="cuda").view(T, topk)
    flat = idx.flatten().to(torch.int64)
    kv_new = torch.randn((T, 1, D), generator=g, device="cuda", dtype=torch.bfloat16)
    slots = idx[:, 0].contiguous()
    new = lambda: ffpa_attn_with_kvcache_mla_sparse_ds(q, pool, DV, idx, softmax_scale=SCALE)
    wide = lambda: ffpa_attn_with_kvcache_mla_sparse(q, pool16, DV, idx, softmax_scale=SCALE)
    fp8 = lambda: ffpa_attn_with_kvcache_mla_sparse_fp8(q, pool8, DV, idx, kv_scale=KV_SCALE, softmax_scale=SCALE)
    store = lambda: store_latent_rows_ds(pool, kv_new, slots)

    def today():
      scratch.copy_(unpack_latent_rows_ds(pool[flat]))  # (gather + unpack in torch: the step's rows, written as twice-and-a-bit their bytes)
      return ffpa_attn_with_kvcache_mla_sparse(q, scratch, DV, ident, softmax_scale=SCALE)

    assert torch.equal(new(), wide())  # (the definition: the two routes return the same bits)
    assert torch.equal(today(), wide())  # (the same rows in another place: the same image)
    plans = plans_of(hip, "mla_sparse_forward", {"A": new, "B": wide, "D": fp8})
    r = interleaved({"A": graphed(new), "B": graphed(wide), "B'": graphed(wide), "C": graphed(today), "D": graphed(fp8), "S": graphed(store)}, args.rounds, args.iters)
    a, b, b2, c, d, s = (r[k][0] for k in ("A", "B", "B'", "C", "D", "S"))
    read = T * topk
    rec = dict(Hq=hq, tokens=T, topk=topk, pool_rows=rows, A_us=round(a, 2), B_us=round(b, 2), Bb_us=round(b2, 2), C_us=round(c, 2), D_us=round(d, 2), S_us=round(s, 2),
               A_over_B=round(a / b, 3), C_over_A=round(c / a, 3), A_over_D=round(a / d, 3), Bb_over_B=round(b2 / b, 4),
               **{f"{k}_min_max": [round(x, 2) for x in r[k][1:]] for k in ("A", "B", "C", "D", "S")}, ds_mib=round(read * ROW / 2 ** 20, 1),
               bf16_mib=round(read * D * 2 / 2 ** 20, 1), A_tbs=round(read * ROW / a / 1e6, 3), B_tbs=round(read * D * 2 / b / 1e6, 3), plan_A=plans["A"], plan_B=plans["B"],
               plan_D=plans["D"])
    out.append(rec)
    print(json.dumps(rec), flush=True)
    del pool, pool16, pool8, scratch
    torch.cuda.empty_cache()
  return out


def write_md(path, recs):
  rows = ["| Hq | shape | A: 656-byte rows us | B: bf16 (floor) us | C: unpack + bf16 us | D: per-tensor fp8 us | S: store us | A / B | C / A | A / D | B' / B (spread) | "
          "rows MiB | bf16 MiB | A TB/s | B TB/s | plan (A) | plan (B) |", "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
  for r in recs:
    rows.append(f"| {r['Hq']} | T {r['tokens']} x topk {r['topk']} of {r['pool_rows']} rows | {r['A_us']} | {r['B_us']} | {r['C_us']} | {r['D_us']} | {r['S_us']} | "
                f"{r['A_over_B']} | {r['C_over_A']} | {r['A_over_D']} | {r['Bb_over_B']} | {r['ds_mib']} | {r['bf16_mib']} | {r['A_tbs']} | {r['B_tbs']} | {r['plan_A']} | "
                f"{r['plan_B']} |")
  with open(path, "w") as f:
    f.write("\n".join(rows) + "\n")


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--rounds", type=int, default=7)
  ap.add_argument("--iters", type=int, default=20)
  ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r25_mla_sparse_ds.json"))
  args = ap.parse_args()
  assert torch.cuda.is_available(), "needs a GPU"
  recs = records(args)
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, "w") as f:
    json.dump({"tool": "tools/gpu_mla_sparse_ds_ab.py", "rounds": args.rounds, "iters": args.iters, "records": recs}, f, indent=1)
  write_md(os.path.splitext(args.out)[0] + "_table.md", recs)


if __name__ == "__main__":
  main()
