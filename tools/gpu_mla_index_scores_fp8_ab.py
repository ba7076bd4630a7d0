"""Developer tool: ``ffpa_mla_index_scores_fp8`` against the 16-bit call and the route a caller of FP8 index keys had before it, and the quantising append
against its torch equivalent (profiles/r36_mla_index_scores_fp8.md).  A measurement, not a gate.

  python tools/gpu_mla_index_scores_fp8_ab.py [--out profiles/r36_mla_index_scores_fp8.json] [--rounds 5] [--iters 20]
        arms per shape on the same tensors, interleaved, warmed, by graph replay — each arm TWICE in the same rounds (x and x'), x' / x being the run-to-run spread
        every ratio is read against:
          (F)   the FP8 call on the packed pool: one launch;
          (H)   the 16-bit call on a bf16 pool dequantised BEFOREHAND (outside the graph): the parent's kernel alone;
          (DH)  the route a caller has today, all of it inside the graph: dequantise the whole pool to bf16 (unpack the planes, codes x scale), then (H);
          (AP)  ffpa_mla_index_k_append_fp8 of the step's keys;   (AT) its torch equivalent: quantize_index_rows and two indexed writes into the planes.

Shapes: tools/gpu_mla_index_scores_ab.py's — 32 sequences of one token over 8k / 32k / 128k keys, 8 x 4 over 32k, one 512-token chunk over 32k; Hi 64, page size
64, a shuffled block table, every length = N, causal off.  K bytes of (F) = sequences x N x 132, of (H) = sequences x N x 256.  Before timing the tool checks (F)
against the definition in float64 on the first token's first 4096 keys.  Every figure is the median of `--rounds` interleaved rounds of `--iters` replays each,
device events: a call's time under graph replay, not a profiler's kernel time."""

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gpu_mla_fp8_sparse_tree_ab import graphed, interleaved  # noqa: E402
from gpu_mla_index_scores_ab import HI, PAGE, SHAPES  # noqa: E402

ARMS = ("F", "H", "DH", "AP", "AT")


def records(args):
  from ffpa_attn_amd import (ffpa_mla_index_k_append_fp8, ffpa_mla_index_scores, ffpa_mla_index_scores_fp8, pack_index_key_pages, quantize_index_rows,
                             unpack_index_key_pages)

  out = []
  for B, Sq, N in SHAPES:
    g = torch.Generator(device="cuda").manual_seed(0)
    T, W = B * Sq, N // PAGE
    codes, scale = quantize_index_rows(torch.randn((B * W, PAGE, 128), generator=g, device="cuda", dtype=torch.bfloat16))
    pool = pack_index_key_pages(codes, scale)
    dequant = lambda: (lambda c, s: (c.float() * s[..., None]).bfloat16())(*unpack_index_key_pages(pool))
    pool16 = dequant()
    table = torch.randperm(B * W, device="cuda", generator=g).to(torch.int32).view(B, W)
    q, qs = quantize_index_rows(torch.randn((T, HI, 128), generator=g, device="cuda", dtype=torch.bfloat16))
    w = torch.randn((T, HI), generator=g, device="cuda") * HI ** -0.5 * qs
    q16 = q.bfloat16()
    lens = torch.full((B,), N, dtype=torch.int32, device="cuda")
    before = lens - Sq
    k_new = torch.randn((T, 128), generator=g, device="cuda", dtype=torch.bfloat16)
    pos = (before.long()[:, None] + torch.arange(Sq, device="cuda")[None]).view(-1)
    page_of, row_of = table.long()[torch.arange(B, device="cuda").repeat_interleave(Sq), pos // PAGE], pos % PAGE
    code_plane, scale_plane = pool.view(B * W, -1)[:, :PAGE * 128].view(B * W, PAGE, 128), pool.view(B * W, -1)[:, PAGE * 128:].view(B * W, PAGE, 4)

    def append_torch():
      c, s = quantize_index_rows(k_new)
      code_plane[page_of, row_of] = c.view(torch.uint8)
      scale_plane[page_of, row_of] = s.view(torch.uint8).view(T, 4)

    fns = dict(F=lambda: ffpa_mla_index_scores_fp8(q, pool, w, lens, table, max_seqlen_k=N, causal=False),
               H=lambda: ffpa_mla_index_scores(q16, pool16, w, lens, table, max_seqlen_k=N, causal=False),
               DH=lambda: ffpa_mla_index_scores(q16, dequant(), w, lens, table, max_seqlen_k=N, causal=False),
               AP=lambda: ffpa_mla_index_k_append_fp8(pool, k_new, before, table), AT=append_torch)
    # the definition in float64 on the first token's first 4096 keys
    keys, q0 = pool16[table[0, :4096 // PAGE].long()].reshape(-1, 128).double(), q16[0].double()  # (scale x codes is exact in bf16: powers of two)
    want = (w[0, :, None].double() * (q0 @ keys.T).clamp(min=0)).sum(0)
    A = (w[0, :, None].abs().double() * (q0.abs() @ keys.abs().T)).sum(0)
    err = float(((fns["F"]()[0, :4096].double() - want).abs() / A).max())
    arms = {}
    for k in ARMS:
      arms[k], arms[k + "'"] = graphed(fns[k]), graphed(fns[k])
    r = interleaved(arms, args.rounds, args.iters)
    rec = dict(sequences=B, tokens_each=Sq, tokens=T, keys=N, Hi=HI, page=PAGE, F_worst_err_over_A=err)
    for k in ARMS:
      rec[f"{k}_us"], rec[f"{k}2_us"] = round(r[k][0], 2), round(r[k + "'"][0], 2)
      rec[f"{k}_min_max"] = [round(x, 2) for x in r[k][1:]]
    rec["H_over_F"], rec["DH_over_F"], rec["AT_over_AP"] = (round(r[a][0] / r[b][0], 3) for a, b in (("H", "F"), ("DH", "F"), ("AT", "AP")))
    rec["F_k_tbs"], rec["H_k_tbs"] = round(B * N * 132 / r["F"][0] / 1e6, 3), round(B * N * 256 / r["H"][0] / 1e6, 3)  # K bytes read once per SEQUENCE
    rec["F_tflops"], rec["H_tflops"] = (round(2.0 * T * N * HI * 128 / r[k][0] / 1e6, 1) for k in ("F", "H"))
    out.append(rec)
    print(json.dumps(rec), flush=True)
    del pool, pool16, codes, arms, fns
    torch.cuda.empty_cache()
  return out


def write_md(path, recs):
  rows = ["| tokens | keys | F: FP8 call us (F') | H: 16-bit call us (H') | DH: dequantise + 16-bit us (DH') | H / F | DH / F | K TB/s of F, H | TFLOP/s of F, H | "
          "append us (') | torch append us (') | worst err / A of F |", "|---|---|---|---|---|---|---|---|---|---|---|---|"]
  for r in recs:
    rows.append(f"| {r['sequences']} x {r['tokens_each']} | {r['keys']} | {r['F_us']} ({r['F2_us']}) | {r['H_us']} ({r['H2_us']}) | {r['DH_us']} ({r['DH2_us']}) | "
                f"{r['H_over_F']} | {r['DH_over_F']} | {r['F_k_tbs']}, {r['H_k_tbs']} | {r['F_tflops']}, {r['H_tflops']} | {r['AP_us']} ({r['AP2_us']}) | "
                f"{r['AT_us']} ({r['AT2_us']}) | {r['F_worst_err_over_A']:.3e} |")
  with open(path, "w") as f:
    f.write("\n".join(rows) + "\n")


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--rounds", type=int, default=5)
  ap.add_argument("--iters", type=int, default=20)
  ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r36_mla_index_scores_fp8.json"))
  args = ap.parse_args()
  assert torch.cuda.is_available(), "needs a GPU"
  recs = records(args)
  os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
  with open(args.out, "w") as f:
    json.dump({"tool": "tools/gpu_mla_index_scores_fp8_ab.py", "rounds": args.rounds, "iters": args.iters, "records": recs}, f, indent=1)
  write_md(os.path.splitext(args.out)[0] + "_table.md", recs)


if __name__ == "__main__":
  main()
