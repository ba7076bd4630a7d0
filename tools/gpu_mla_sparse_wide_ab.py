"""Developer tool: what the WIDE builds of the three sparse latent calls (``wide_pool=True``: 64-bit lane addresses) cost against the narrow builds, and the point the
narrow builds could not reach — a latent pool of 32 x 128k rows (profiles/r37_mla_sparse_wide.md).  A measurement, not a gate.

  python tools/gpu_mla_sparse_wide_ab.py [--out profiles/r37_mla_sparse_wide.json] [--rounds 7] [--iters 20] [--part ab|far|chain ...]
    every arm by graph replay on the SAME tensors, interleaved, warmed, and TWICE (k and k'): k' / k is the run's own spread, which the ratios are read against.
    (ab)    T 32 x topk 2048 slots drawn from a pool of 32 x 32k rows, Hq 16 and 128, the three pool kinds: (N) wide_pool=False, (W) wide_pool=True.
    (far)   the same step over a pool of 32 x 128k rows — past 2^31 bytes per head in every kind: (W) the wide call on the pool, (G) the route such a pool needed
            before — torch.index_select of the selected rows into a scratch pool + the NARROW call of the kind over it with the identity list.
    (chain) 32 sequences x 128k keys, one token each: ffpa_mla_index_scores -> ffpa_mla_sparse_topk_slots -> the wide 16-bit sparse call in ONE graph (C), next to
            the first two launches alone (S).
  Writes the records as JSON and, next to it, `<out>_table.md`."""

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

T, TOPK, PAGE, D, DV, HI = 32, 2048, 64, 576, 512, 64
SCALE, KV_SCALE = 192 ** -0.5, 0.5
KINDS = ("16bit", "fp8", "ds")


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


def interleaved(fns: dict, rounds, iters):
  """Every arm twice (k, k'), in rounds -> {k: median us}, {k: k' / k}."""
  arms = {}
  for k, fn in fns.items():
    arms[k], arms[k + "'"] = graphed(fn), graphed(fn)
  for run in arms.values():
    time_us(run, iters)
  samples = {k: [] for k in arms}
  for _ in range(rounds):
    for k, run in arms.items():
      samples[k].append(time_us(run, iters))
  med = {k: statistics.median(v) for k, v in samples.items()}
  return {k: round(med[k], 2) for k in fns}, {k: round(med[k + "'"] / med[k], 4) for k in fns}


def make_pool(kind, rows, g):
  """A pool of `rows` random latent rows of the kind (filled in slices: the float32 draw of 4 M rows would not be small) and the kind's public call."""
  import ffpa_attn_amd as F

  dt = {"16bit": torch.bfloat16, "fp8": torch.float8_e4m3fn, "ds": torch.uint8}[kind]
  pool = torch.empty((rows, 1, 656 if kind == "ds" else D), device="cuda", dtype=dt)
  for r0 in range(0, rows, 1 << 18):
    x = torch.randn((min(1 << 18, rows - r0), 1, D), generator=g, device="cuda")
    pool[r0:r0 + x.size(0)] = F.pack_latent_rows_ds(x.to(torch.bfloat16)) if kind == "ds" else (x / KV_SCALE).to(dt) if kind == "fp8" else x.to(dt)
  fn, kw = {"16bit": (F.ffpa_attn_with_kvcache_mla_sparse, {}), "fp8": (F.ffpa_attn_with_kvcache_mla_sparse_fp8, dict(kv_scale=KV_SCALE)),
            "ds": (F.ffpa_attn_with_kvcache_mla_sparse_ds, {})}[kind]
  return pool, lambda q, p, idx, lens, wide: fn(q, p, DV, idx, topk_lens=lens, softmax_scale=SCALE, wide_pool=wide, **kw)


def step(hq, rows, g):
  q = torch.randn((T, hq, D), generator=g, device="cuda", dtype=torch.bfloat16)
  idx = torch.randint(0, rows, (T, TOPK), generator=g, device="cuda", dtype=torch.int32)
  return q, idx, torch.full((T,), TOPK, dtype=torch.int32, device="cuda")


def part_ab(args):
  out, rows = [], 32 * 32 * 1024
  for kind in KINDS:
    g = torch.Generator(device="cuda").manual_seed(1)
    pool, call = make_pool(kind, rows, g)
    for hq in (16, 128):
      q, idx, lens = step(hq, rows, g)
      assert torch.equal(call(q, pool, idx, lens, True), call(q, pool, idx, lens, False))  # (the bits of the narrow build)
      us, spread = interleaved({"N": lambda: call(q, pool, idx, lens, False), "W": lambda: call(q, pool, idx, lens, True)}, args.rounds, args.iters)
      out.append(dict(part="ab", kind=kind, Hq=hq, rows=rows, narrow_us=us["N"], wide_us=us["W"], wide_over_narrow=round(us["W"] / us["N"], 4),
                      spread_narrow=spread["N"], spread_wide=spread["W"]))
      print(json.dumps(out[-1]), flush=True)
    del pool
    torch.cuda.empty_cache()
  return out


def part_far(args):
  out, rows = [], 32 * 128 * 1024
  for kind in KINDS:
    g = torch.Generator(device="cuda").manual_seed(2)
    pool, call = make_pool(kind, rows, g)
    scratch = torch.empty((T * TOPK,) + tuple(pool.shape[1:]), device="cuda", dtype=pool.dtype)
    ident = torch.arange(T * TOPK, device="cuda", dtype=torch.int32).view(T, TOPK)
    raw = lambda t: t.view(torch.uint8)  # (index_select knows no float8)
    for hq in (16, 128):
      q, idx, lens = step(hq, rows, g)
      flat_idx = idx.view(-1)

      def gather():
        torch.index_select(raw(pool), 0, flat_idx, out=raw(scratch))
        return call(q, scratch, ident, lens, False)

      assert torch.equal(call(q, pool, idx, lens, True), gather())  # (the two routes compute the same bits)
      us, spread = interleaved({"W": lambda: call(q, pool, idx, lens, True), "G": gather}, args.rounds, args.iters)
      out.append(dict(part="far", kind=kind, Hq=hq, rows=rows, pool_gib=round(pool.numel() * pool.element_size() / 2 ** 30, 2), wide_us=us["W"], gather_us=us["G"],
                      gather_over_wide=round(us["G"] / us["W"], 3), spread_wide=spread["W"], spread_gather=spread["G"]))
      print(json.dumps(out[-1]), flush=True)
    del pool, scratch
    torch.cuda.empty_cache()
  return out


def part_chain(args):
  from ffpa_attn_amd import ffpa_attn_with_kvcache_mla_sparse, ffpa_mla_index_scores, ffpa_mla_sparse_topk_slots

  B, N, hq = 32, 128 * 1024, 128
  W = N // PAGE
  g = torch.Generator(device="cuda").manual_seed(3)
  keys = torch.randn((B * W, PAGE, 128), generator=g, device="cuda", dtype=torch.bfloat16)
  latent = make_pool("16bit", B * N, g)[0].view(B * W, PAGE, 1, D)
  table = torch.randperm(B * W, device="cuda", generator=g).to(torch.int32).view(B, W)
  qi = torch.randn((B, HI, 128), generator=g, device="cuda", dtype=torch.bfloat16)
  ql = torch.randn((B, hq, D), generator=g, device="cuda", dtype=torch.bfloat16)
  w = torch.randn((B, HI), generator=g, device="cuda") * HI ** -0.5
  lens = torch.full((B,), N, dtype=torch.int32, device="cuda")
  select = lambda: ffpa_mla_sparse_topk_slots(ffpa_mla_index_scores(qi, keys, w, lens, table, max_seqlen_k=N, causal=False), TOPK, lens, table, PAGE, causal=False)

  def chain():
    idx, n = select()
    return ffpa_attn_with_kvcache_mla_sparse(ql, latent, DV, idx, topk_lens=n, softmax_scale=SCALE, wide_pool=True)

  us, spread = interleaved({"S": select, "C": chain}, args.rounds, args.iters)
  rec = dict(part="chain", sequences=B, keys=N, Hq=hq, Hi=HI, topk=TOPK, latent_gib=round(latent.numel() * 2 / 2 ** 30, 2), scores_select_us=us["S"], chain_us=us["C"],
             spread_select=spread["S"], spread_chain=spread["C"])
  print(json.dumps(rec), flush=True)
  return [rec]


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--rounds", type=int, default=7)
  ap.add_argument("--iters", type=int, default=20)
  ap.add_argument("--part", nargs="+", default=["ab", "far", "chain"], choices=["ab", "far", "chain"])
  ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r37_mla_sparse_wide.json"))
  args = ap.parse_args()
  assert torch.cuda.is_available(), "needs a GPU"
  records = [r for p in args.part for r in {"ab": part_ab, "far": part_far, "chain": part_chain}[p](args)]
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, "w") as f:
    json.dump({"tool": "tools/gpu_mla_sparse_wide_ab.py", "rounds": args.rounds, "iters": args.iters, "records": records}, f, indent=1)
  with open(os.path.splitext(args.out)[0] + "_table.md", "w") as f:
    for part in args.part:
      rows = [r for r in records if r["part"] == part]
      cols = [k for k in rows[0] if k != "part"]
      f.write(f"part {part}\n\n| " + " | ".join(cols) + " |\n|" + "---|" * len(cols) + "\n" + "".join("| " + " | ".join(str(r[c]) for c in cols) + " |\n" for r in rows) + "\n")


if __name__ == "__main__":
  main()
