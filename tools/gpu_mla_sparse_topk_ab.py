"""Developer tool: ``ffpa_mla_sparse_topk_slots`` against the route a caller had before it, alone and in front of the 16-bit sparse latent call
(profiles/r32_mla_sparse_topk.md).  A measurement, not a gate.

  python tools/gpu_mla_sparse_topk_ab.py [--out profiles/r32_mla_sparse_topk.json] [--rounds 5] [--iters 50]
        arms per shape on the same scores, lengths and block table, interleaved, warmed, by graph replay — each arm TWICE in the same rounds (x and x'), x' / x
        being the run-to-run spread every ratio is read against:
          (A)  the new call: one launch;
          (P)  the parent commit's route, all of it inside the graph: torch.topk over [T, N], the gather of the block table to one row per token,
               slots_from_block_table, compact_topk_indices;
          (AS) (A) followed by ffpa_attn_with_kvcache_mla_sparse on its pair;   (PS) (P) followed by the same call on its pair.
        Writes the records as JSON and a markdown table next to it.

Shapes: T = 32 tokens (32 sequences of one token) x topk 2048 over 8k / 32k columns, 8 sequences of 4 tokens over 128k columns, and one 512-token chunk of one
sequence over 32k columns (profiles/r19_mla_sparse.md's step and its neighbours); page size 64, a shuffled block table, every length = N and causal off — every
token sees every column, which is what the parent's route computes without a masking launch more.  Hq 16, D = 576, head_dim_v = 512, bf16, pool of B x N rows.
Before timing the tool checks that both routes select the SAME SET of slots per token (their order differs: ascending positions here, torch.topk's there) and
that the new call's pair equals the definition's.  Every figure is the median of `--rounds` interleaved rounds of `--iters` replays each, device events."""

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))

from gpu_mla_fp8_sparse_tree_ab import graphed, interleaved  # noqa: E402

D, DV, PAGE, HQ = 576, 512, 64, 16
SCALE = 192 ** -0.5
SHAPES = [(32, 1, 2048, 8192), (32, 1, 2048, 32768), (8, 4, 2048, 131072), (1, 512, 2048, 32768)]  # (sequences, tokens of each, topk, columns)
ARMS = ("A", "P", "AS", "PS")


def records(args):
  import kvcache_mla_sparse_topk_ref as TR
  from ffpa_attn_amd import compact_topk_indices, ffpa_attn_with_kvcache_mla_sparse, ffpa_mla_sparse_topk_slots, slots_from_block_table

  out = []
  for B, Sq, topk, N in SHAPES:
    g = torch.Generator(device="cuda").manual_seed(0)
    T, W = B * Sq, N // PAGE
    pool = torch.randn((B * W, PAGE, 1, D), generator=g, device="cuda", dtype=torch.bfloat16)
    table = torch.randperm(B * W, device="cuda", generator=g).to(torch.int32).view(B, W)
    scores = torch.randn((T, N), generator=g, device="cuda")
    lens = torch.full((B,), N, dtype=torch.int32, device="cuda")
    seq = torch.arange(T, device="cuda") // Sq
    q = torch.randn((T, HQ, D), generator=g, device="cuda", dtype=torch.bfloat16)
    attend = lambda pair: ffpa_attn_with_kvcache_mla_sparse(q, pool, DV, pair[0], topk_lens=pair[1], softmax_scale=SCALE)
    new = lambda: ffpa_mla_sparse_topk_slots(scores, topk, lens, table, PAGE, causal=False)
    parent = lambda: compact_topk_indices(slots_from_block_table(torch.topk(scores, topk, dim=1).indices, table[seq], PAGE))
    (a_idx, a_n), (p_idx, p_n) = new(), parent()
    assert torch.equal(a_n, p_n) and torch.equal(a_idx.sort(dim=1).values, p_idx.sort(dim=1).values)  # (the same set of slots per token)
    few = min(T, 8)  # (the definition runs on the CPU: the first rows, each as a sequence of one token with its sequence's table row — causal off, so n = N)
    want = TR.topk_slots(scores[:few].cpu(), topk, torch.full((few,), N, dtype=torch.int32), table[seq[:few]].cpu(), PAGE, causal=False)
    assert torch.equal(a_idx[:few].cpu(), want[0]) and torch.equal(a_n[:few].cpu(), want[1])
    arms = {}
    for k, fn in (("A", new), ("P", parent), ("AS", lambda: attend(new())), ("PS", lambda: attend(parent()))):
      arms[k], arms[k + "'"] = graphed(fn), graphed(fn)
    r = interleaved(arms, args.rounds, args.iters)
    rec = dict(sequences=B, tokens_each=Sq, tokens=T, topk=topk, columns=N, page=PAGE, Hq=HQ)
    for k in ARMS:
      rec[f"{k}_us"], rec[f"{k}2_us"] = round(r[k][0], 2), round(r[k + "'"][0], 2)
      rec[f"{k}_min_max"] = [round(x, 2) for x in r[k][1:]]
      rec[f"{k}_spread"] = round(r[k + "'"][0] / r[k][0], 4)
    rec["P_over_A"], rec["PS_over_AS"] = round(r["P"][0] / r["A"][0], 3), round(r["PS"][0] / r["AS"][0], 3)
    rec["score_mib"] = round(T * N * 4 / 2 ** 20, 1)
    out.append(rec)
    print(json.dumps(rec), flush=True)
    del pool, scores, arms
    torch.cuda.empty_cache()
  return out


def write_md(path, recs):
  rows = ["| tokens | columns | topk | scores MiB | A: one launch us (A') | P: parent route us (P') | P / A | A + sparse us (') | P + sparse us (') | PS / AS | "
          "spread A' / A, P' / P, AS' / AS, PS' / PS |", "|---|---|---|---|---|---|---|---|---|---|---|"]
  for r in recs:
    rows.append(f"| {r['sequences']} x {r['tokens_each']} | {r['columns']} | {r['topk']} | {r['score_mib']} | {r['A_us']} ({r['A2_us']}) | {r['P_us']} ({r['P2_us']}) | "
                f"{r['P_over_A']} | {r['AS_us']} ({r['AS2_us']}) | {r['PS_us']} ({r['PS2_us']}) | {r['PS_over_AS']} | "
                f"{r['A_spread']}, {r['P_spread']}, {r['AS_spread']}, {r['PS_spread']} |")
  with open(path, "w") as f:
    f.write("\n".join(rows) + "\n")


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--rounds", type=int, default=5)
  ap.add_argument("--iters", type=int, default=50)
  ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r32_mla_sparse_topk.json"))
  args = ap.parse_args()
  assert torch.cuda.is_available(), "needs a GPU"
  recs = records(args)
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, "w") as f:
    json.dump({"tool": "tools/gpu_mla_sparse_topk_ab.py", "rounds": args.rounds, "iters": args.iters, "records": recs}, f, indent=1)
  write_md(os.path.splitext(args.out)[0] + "_table.md", recs)


if __name__ == "__main__":
  main()
