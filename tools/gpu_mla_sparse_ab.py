"""Developer tool: what the sparse (top-k indexed) latent call costs against the route a caller had before it and against its floor (profiles/r19_mla_sparse.md).

  python tools/gpu_mla_sparse_ab.py [--out profiles/r19_mla_sparse.json] [--rounds 7] [--iters 20]
        arms per shape on the SAME tensors, interleaved, warmed, by graph replay:
          (sparse)  ffpa_attn_with_kvcache_mla_sparse(q, pool, 512, indices): the rows are read where they lie;
          (sparse2) the same arm again, as an arm of its own in the same rounds: sparse2 / sparse is the run-to-run spread the ratios are read against;
          (gather)  torch.index_select of the selected rows into a [T, topk, 1, 576] scratch cache + ffpa_attn_with_kvcache_mla on it: the route a caller had —
                    every selected row is read, written and read again, and there is a launch more;
          (floor)   ffpa_attn_with_kvcache_mla alone on that already-gathered cache: what attention over topk contiguous rows costs.
        Writes the records as JSON and a markdown table next to it.

Shapes: T = 32 tokens x topk = 2048 slots drawn without order from pools of 32 x 32k and 32 x 128k rows (page size 64), Hq 16 and Hq 128 on one latent head, D = 576,
head_dim_v = 512, bf16, scale 1 / sqrt(192).  A pool whose rows span more than 2^31 bytes is refused by the sparse call (its 32-bit offsets): that arm is then
recorded as REFUSED and the other two are still measured.  Every figure is the median of `--rounds` interleaved rounds of `--iters` replays each, timed with
device events."""

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

T, TOPK, PAGE, D, DV = 32, 2048, 64, 576, 512
SCALE = 192 ** -0.5
SHAPES = [(hq, rows) for rows in (32 * 32 * 1024, 32 * 128 * 1024) for hq in (16, 128)]  # (Hq, rows of the pool)


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
  rows = ["| Hq | pool rows | pool GiB | sparse us | gather us | floor us | gather / sparse | sparse / floor | sparse2 / sparse (spread) | plan (sparse) | plan (floor) |",
          "|---|---|---|---|---|---|---|---|---|---|---|"]
  for r in records:
    rows.append(f"| {r['Hq']} | {r['rows']} | {r['pool_gib']} | {r['sparse_us']} | {r['gather_us']} | {r['floor_us']} | {r['gather_over_sparse']} | {r['sparse_over_floor']} | "
                f"{r['sparse2_over_sparse']} | {r['plan_sparse']} | {r['plan_floor']} |")
  with open(path, "w") as f:
    f.write("\n".join(rows) + "\n")


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--rounds", type=int, default=7)
  ap.add_argument("--iters", type=int, default=20)
  ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r19_mla_sparse.json"))
  args = ap.parse_args()
  from ffpa_attn_amd import ffpa_attn_with_kvcache_mla, ffpa_attn_with_kvcache_mla_sparse, hip

  assert torch.cuda.is_available(), "needs a GPU"
  records = []
  for hq, rows in SHAPES:
    g = torch.Generator(device="cuda").manual_seed(rows + hq)
    pool = torch.empty((rows // PAGE, PAGE, 1, D), device="cuda", dtype=torch.bfloat16).normal_(generator=g)
    flat = pool.view(rows, 1, D)
    q = torch.randn((T, hq, D), generator=g, device="cuda", dtype=torch.bfloat16)
    idx = torch.randint(0, rows, (T, TOPK), generator=g, device="cuda", dtype=torch.int32)
    lens = torch.full((T,), TOPK, dtype=torch.int32, device="cuda")
    scratch = torch.empty((T, TOPK, 1, D), device="cuda", dtype=torch.bfloat16)
    flat_idx = idx.view(-1)

    def gather():
      torch.index_select(flat, 0, flat_idx, out=scratch.view(T * TOPK, 1, D))
      return ffpa_attn_with_kvcache_mla(q[:, None], scratch, DV, cache_seqlens=lens, softmax_scale=SCALE)

    floor = lambda: ffpa_attn_with_kvcache_mla(q[:, None], scratch, DV, cache_seqlens=lens, softmax_scale=SCALE)
    sparse = lambda: ffpa_attn_with_kvcache_mla_sparse(q, pool, DV, idx, topk_lens=lens, softmax_scale=SCALE)
    want = gather()[:, 0]
    refused = None
    try:
      torch.testing.assert_close(sparse().float(), want.float(), atol=2e-2, rtol=2e-2)  # (the routes compute the same thing)
    except ValueError as e:
      refused = str(e)
    plans = {}
    real_mla, real_sp = hip.mla_forward, hip.mla_sparse_forward
    for key, real, name in (("floor", real_mla, "mla_forward"), ("sparse", real_sp, "mla_sparse_forward")):
      def spy(*a, _real=real, _key=key, **kw):
        kw["plan_out"] = plans.setdefault(_key, {})
        return _real(*a, **kw)
      setattr(hip, name, spy)
    try:
      floor()
      if refused is None:
        sparse()
    finally:
      hip.mla_forward, hip.mla_sparse_forward = real_mla, real_sp
    brief = lambda p: f"{p['workgroups']} wg, {p['row_tiles']} row tiles, {p['splits']} splits{', NT' if ', NT>' in p['kernel'] else ''}"
    arms = {"gather": graphed(gather), "floor": graphed(floor)}
    if refused is None:
      arms.update({"sparse": graphed(sparse), "sparse2": graphed(sparse)})
    r = interleaved(arms, args.rounds, args.iters)
    us = lambda k: round(r[k][0], 2) if k in r else "REFUSED"
    ratio = lambda a, b, nd=3: round(r[a][0] / r[b][0], nd) if a in r and b in r else "REFUSED"
    rec = {"Hq": hq, "T": T, "topk": TOPK, "rows": rows, "pool_gib": round(rows * D * 2 / 2 ** 30, 2), "sparse_us": us("sparse"), "sparse2_us": us("sparse2"),
           "gather_us": us("gather"), "floor_us": us("floor"), "gather_over_sparse": ratio("gather", "sparse"), "sparse_over_floor": ratio("sparse", "floor"),
           "sparse2_over_sparse": ratio("sparse2", "sparse", 4), "min_max": {k: [round(x, 2) for x in v[1:]] for k, v in r.items()},
           "selected_mib": round(T * TOPK * D * 2 / 2 ** 20, 1), "plan_sparse": brief(plans["sparse"]) if refused is None else "REFUSED", "plan_floor": brief(plans["floor"]),
           "refused": refused}
    records.append(rec)
    print(json.dumps(rec), flush=True)
    del pool, flat, q, idx, scratch, arms
    torch.cuda.empty_cache()
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, "w") as f:
    json.dump({"tool": "tools/gpu_mla_sparse_ab.py", "rounds": args.rounds, "iters": args.iters, "records": records}, f, indent=1)
  write_md(os.path.splitext(args.out)[0] + "_table.md", records)


if __name__ == "__main__":
  main()
