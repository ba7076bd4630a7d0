"""Developer tool: ``ffpa_mla_index_scores`` against the route a caller had before it, the sweep of its chunk size, and the three-launch chain it opens
(profiles/r35_mla_index_scores.md).  A measurement, not a gate.

  python tools/gpu_mla_index_scores_ab.py [--out profiles/r35_mla_index_scores.json] [--rounds 5] [--iters 20]
        arms per shape on the same tensors, interleaved, warmed, by graph replay — each arm TWICE in the same rounds (x and x'), x' / x being the run-to-run spread
        every ratio is read against:
          (A)    the new call: one launch, the chunk the library ships (hip.MLA_INDEX_CHUNK_KEYS);
          (P)    the torch route, all of it inside the graph: the gather of every sequence's index keys by the block table, einsum, relu, the multiply by the
                 head weights, the sum over heads, the -inf fill;
          (C256) (C512) (C1024)  the new launch with chunk_keys = 256 / 512 / 1024 (the sweep);
          (ASS)  (A) followed by ffpa_mla_sparse_topk_slots and ffpa_attn_with_kvcache_mla_sparse: the chain of a DeepSeek-V3.2 layer (where the latent pool
                 of the shape stays inside the sparse call's 2^31 bytes).
        Writes the records as JSON and, next to it, `<out>_table.md`: the raw table the hand-written profiles/r35_mla_index_scores.md quotes (not that file).

Shapes: 32 sequences of one token over 8k / 32k / 128k keys, 8 sequences of 4 tokens over 32k, one 512-token chunk of one sequence over 32k; Hi 64, bf16, page size
64, a shuffled block table, every length = N.  Every shape runs causal off (every token sees every key: what the torch route computes without
a masking launch more — its -inf fill is then a no-op that is still launched); K bytes = sequences x N x 256, the least a one-token step must read.  Before
timing the tool checks the new call against the definition in float64 on the first rows.  Every figure is the median of `--rounds` interleaved rounds of `--iters`
replays each, device events."""

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gpu_mla_fp8_sparse_tree_ab import graphed, interleaved  # noqa: E402

HI, PAGE, TOPK, D, DV, HQ = 64, 64, 2048, 576, 512, 16
SHAPES = [(32, 1, 8192), (32, 1, 32768), (32, 1, 131072), (8, 4, 32768), (1, 512, 32768)]  # (sequences, tokens of each, keys)
ARMS = ("A", "P", "C256", "C512", "C1024", "ASS")


def torch_route(q, pool, w, lens, table, N, Sq):
  """What a caller runs today: gather, einsum, relu, weight, sum, -inf pad -> float32 [T, N]."""
  B = table.size(0)
  keys = pool[table.long()].reshape(B, -1, 128)[:, :N]  # the gathered copy of the whole index-key cache
  s = torch.einsum("bshd,bnd->bshn", q.view(B, Sq, HI, 128), keys).float().relu_()
  s = (s * w.view(B, Sq, HI, 1)).sum(2)
  seen = torch.arange(N, device=q.device)[None, None, :] < lens[:, None, None]
  return s.masked_fill_(~seen, float("-inf")).view(B * Sq, N)


def records(args):
  from ffpa_attn_amd import ffpa_attn_with_kvcache_mla_sparse, ffpa_mla_index_scores, ffpa_mla_sparse_topk_slots, hip

  out = []
  for B, Sq, N in SHAPES:
    g = torch.Generator(device="cuda").manual_seed(0)
    T, W = B * Sq, N // PAGE
    pool = torch.randn((B * W, PAGE, 128), generator=g, device="cuda", dtype=torch.bfloat16)
    chained = B * N * D * 2 <= 2 ** 31  # (the sparse call's 32-bit offsets reach 2^31 bytes of pool: no chain at 32 x 128k)
    latent = torch.randn((B * W, PAGE, 1, D), generator=g, device="cuda", dtype=torch.bfloat16) if chained else None
    table = torch.randperm(B * W, device="cuda", generator=g).to(torch.int32).view(B, W)
    q = torch.randn((T, HI, 128), generator=g, device="cuda", dtype=torch.bfloat16)
    ql = torch.randn((T, HQ, D), generator=g, device="cuda", dtype=torch.bfloat16)
    w = torch.randn((T, HI), generator=g, device="cuda") * HI ** -0.5
    lens = torch.full((B,), N, dtype=torch.int32, device="cuda")
    new = lambda: ffpa_mla_index_scores(q, pool, w, lens, table, max_seqlen_k=N, causal=False)
    chunked = lambda c: (lambda: hip.mla_index_scores(q, pool, w, lens, table, N, None, False, chunk_keys=c))
    parent = lambda: torch_route(q, pool, w, lens, table, N, Sq)

    def chain():
      idx, n = ffpa_mla_sparse_topk_slots(new(), TOPK, lens, table, PAGE, causal=False)
      return ffpa_attn_with_kvcache_mla_sparse(ql, latent, DV, idx, topk_lens=n, softmax_scale=192 ** -0.5)

    # the definition in float64 on the first token's first 4096 keys, against every chunk size
    keys = pool[table[0, :4096 // PAGE].long()].reshape(-1, 128).double()
    want = (w[0, :, None].double() * (q[0].double() @ keys.T).clamp(min=0)).sum(0)
    bound = (128 + HI + 8) * 2.0 ** -23 * (w[0, :, None].abs().double() * (q[0].abs().double() @ keys.abs().T)).sum(0)
    for fn in (new, chunked(256), chunked(512), chunked(1024)):
      assert bool(((fn()[0, :4096].double() - want).abs() <= bound).all())
    arms = {}
    for k, fn in (("A", new), ("P", parent), ("C256", chunked(256)), ("C512", chunked(512)), ("C1024", chunked(1024))) + ((("ASS", chain),) if chained else ()):
      arms[k], arms[k + "'"] = graphed(fn), graphed(fn)
    r = interleaved(arms, args.rounds, args.iters)
    rec = dict(sequences=B, tokens_each=Sq, tokens=T, keys=N, Hi=HI, page=PAGE, topk=TOPK, chunk_keys=hip.MLA_INDEX_CHUNK_KEYS)
    for k in ARMS:
      if k + "'" not in arms:
        rec[f"{k}_us"] = rec[f"{k}2_us"] = "NOT MEASURED"
        continue
      rec[f"{k}_us"], rec[f"{k}2_us"] = round(r[k][0], 2), round(r[k + "'"][0], 2)
      rec[f"{k}_min_max"] = [round(x, 2) for x in r[k][1:]]
      rec[f"{k}_spread"] = round(r[k + "'"][0] / r[k][0], 4)
    rec["P_over_A"] = round(r["P"][0] / r["A"][0], 3)
    rec["k_mib"] = round(B * N * 256 / 2 ** 20, 1)
    rec["A_k_tbs"] = round(B * N * 256 / r["A"][0] / 1e6, 3)  # K bytes read once per SEQUENCE over the call's time
    rec["A_tflops"] = round(2.0 * T * N * HI * 128 / r["A"][0] / 1e6, 1)
    out.append(rec)
    print(json.dumps(rec), flush=True)
    del pool, latent, arms
    torch.cuda.empty_cache()
  return out


def write_md(path, recs):
  rows = ["| tokens | keys | K MiB | A: one launch us (A') | P: torch route us (P') | P / A | K TB/s of A | TFLOP/s of A | C256 us (') | C512 us (') | C1024 us (') | "
          "A + selection + sparse us (') | spread A' / A, P' / P |", "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
  for r in recs:
    rows.append(f"| {r['sequences']} x {r['tokens_each']} | {r['keys']} | {r['k_mib']} | {r['A_us']} ({r['A2_us']}) | {r['P_us']} ({r['P2_us']}) | {r['P_over_A']} | "
                f"{r['A_k_tbs']} | {r['A_tflops']} | {r['C256_us']} ({r['C2562_us']}) | {r['C512_us']} ({r['C5122_us']}) | {r['C1024_us']} ({r['C10242_us']}) | "
                f"{r['ASS_us']} ({r['ASS2_us']}) | {r['A_spread']}, {r['P_spread']} |")
  with open(path, "w") as f:
    f.write("\n".join(rows) + "\n")


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--rounds", type=int, default=5)
  ap.add_argument("--iters", type=int, default=20)
  ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r35_mla_index_scores.json"))
  args = ap.parse_args()
  assert torch.cuda.is_available(), "needs a GPU"
  recs = records(args)
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, "w") as f:
    json.dump({"tool": "tools/gpu_mla_index_scores_ab.py", "rounds": args.rounds, "iters": args.iters, "records": recs}, f, indent=1)
  write_md(os.path.splitext(args.out)[0] + "_table.md", recs)


if __name__ == "__main__":
  main()
