"""The gap budget of the single-tile prefill loops (csrc/ffpa_fwd_m16_tile.inc, FFPA_M16_GAP_SPLIT), read off the assembly build() keeps.

One K / V^T fragment feeds a PAIR of MFMAs (the two 16-row halves), so a fragment's bookkeeping — the LDS reads that request a later fragment, the counted wait
for this one, and on some pairs a DMA piece's M0 write and its buffer_load — has two MFMA gaps to sit in.  One wave per SIMD hides one or two single-issue
instructions in a gap and pays for the third (profiles/r06_gap_probe.txt, profiles/r30_gap_budget.md), so the loops deal them over both gaps:

    PV     {ds_read_b64_tr_b16, s_waitcnt [, s_add_u32 m0]}  MFMA   {[buffer_load ... lds,] ds_read_b64_tr_b16}   MFMA      at most 3 per gap
    QK^T   {ds_read_b128, s_waitcnt [, s_add_u32 m0]}        MFMA   {[buffer_load ... lds]}                       MFMA      at most 3 per gap

(the PV loop of the parent kept both transpose reads in front of the first MFMA: 4 in a gap of a pair with a piece, two transpose reads in one gap — it fails
the first two tests.  The QK^T loop keeps the parent's form: one read per pair, and moving it measured nothing.)
Skipped when the assembly files are not there, like tests/test_isa_rules.py.
"""
import glob
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEMPS = glob.glob(os.path.join(ROOT, "ffpa_attn_amd", "csrc", "build", "temps_d512", "*gfx950.s*"))  # (.s, or .s.gz as build() leaves them)
pytestmark = pytest.mark.skipif(not TEMPS, reason="no --save-temps assembly in csrc/build")

# non-MFMA instructions (s_nop and waits included) the shipped form puts in one gap between two consecutive MFMAs of a loop, from the final assembly
QK_GAP_MAX = 3
PV_GAP_MAX = 3

HEADLINE = {"bf16": "_ZN4ffpa19ffpa_fwd_m16_kernelIDF16bLi512ELi0ELb0EEEvNS_7FwdArgsE", "fp16": "_ZN4ffpa19ffpa_fwd_m16_kernelIDF16_Li512ELi0ELb0EEEvNS_7FwdArgsE"}
PACKED = {"bf16": "_ZN4ffpa26ffpa_fwd_m16_varlen_kernelIDF16bLi512ELb0EEEvNS_7FwdArgsENS_10VarlenArgsE",
          "fp16": "_ZN4ffpa26ffpa_fwd_m16_varlen_kernelIDF16_Li512ELb0EEEvNS_7FwdArgsENS_10VarlenArgsE"}


def _isa_stats():
  spec = importlib.util.spec_from_file_location("isa_stats", os.path.join(ROOT, "tools", "isa_stats.py"))
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  return mod


_BODIES = {}


def _body(symbol):
  """The kernel's instructions, one mnemonic + operands per entry: no comment lines, no ;;#ASMSTART / ;;#ASMEND fences, no labels, no directives."""
  if not _BODIES:
    st = _isa_stats()
    for path in st.isa_files(512):
      for name, body in st.kernels(path):
        _BODIES[name] = body
  assert symbol in _BODIES, f"{symbol} is not in the D = 512 assembly"
  out = []
  for line in _BODIES[symbol]:
    s = line.split(";")[0].strip()
    if s and not s.endswith(":") and not s.startswith("."):
      out.append(s)
  return out


def _loops(ins):
  """The MFMA loops of a kernel: runs of MFMAs less than 16 instructions apart (the loops' gaps hold a handful; the softmax between them > 100), as lists of
  gaps — the instructions between two consecutive MFMAs of the run."""
  loops, gaps, cur, since = [], [], [], None
  for s in ins:
    if s.startswith("v_mfma"):
      if since is not None and since > 16:
        loops.append(gaps)
        gaps = []
      elif since is not None:
        gaps.append(cur)
      cur, since = [], 0
    elif since is not None:
      cur.append(s)
      since += 1
  loops.append(gaps)
  return loops


def _qk_and_pv(symbol):
  loops = _loops(_body(symbol))
  assert [len(g) + 1 for g in loops] == [128, 128], [len(g) + 1 for g in loops]  # QK^T and PV of the one KV step: 64 fragment pairs each
  qk, pv = loops
  assert any(i.startswith("ds_read_b128") for g in qk for i in g) and not any("_tr_" in i for g in qk for i in g)
  assert any(i.startswith("ds_read_b64_tr_b16") for g in pv for i in g) and not any(i.startswith("ds_read_b128") for g in pv for i in g)
  return qk, pv


KERNELS = [("headline-bf16", HEADLINE["bf16"]), ("headline-fp16", HEADLINE["fp16"]), ("packed-bf16", PACKED["bf16"]), ("packed-fp16", PACKED["fp16"])]


@pytest.mark.parametrize("symbol", [k[1] for k in KERNELS], ids=[k[0] for k in KERNELS])
def test_no_mfma_gap_holds_more_than_the_shipped_form_puts_there(symbol):
  qk, pv = _qk_and_pv(symbol)
  worst_qk, worst_pv = max(qk, key=len), max(pv, key=len)
  print(f"QK^T: largest gap {len(worst_qk)} {worst_qk}; PV: largest gap {len(worst_pv)} {worst_pv}")
  assert len(worst_qk) <= QK_GAP_MAX, worst_qk
  assert len(worst_pv) <= PV_GAP_MAX, worst_pv


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_every_pv_gap_of_the_headline_kernel_holds_at_most_one_transpose_read(dtype):
  _, pv = _qk_and_pv(HEADLINE[dtype])
  per_gap = [sum(i.startswith("ds_read_b64_tr_b16") for i in g) for g in pv]
  assert max(per_gap) == 1, per_gap
  # every fragment but the FFPA_M16_PF2 = 4 requested in front of the loop is requested inside it, two reads each; the first of them stands in front of the loop's first MFMA
  assert sum(per_gap) == 2 * (64 - 4) - 1, sum(per_gap)


def test_the_headline_kernel_keeps_its_registers(monkeypatch, capsys):
  """What tools/isa_stats.py reported before the reads moved: no scratch, 256 MFMAs per KV step, O^T = the 256 AGPRs."""
  import sys

  monkeypatch.setattr(sys, "argv", ["isa_stats", "512"])
  _isa_stats().main()
  lines = capsys.readouterr().out.splitlines()
  for tag in ("m16 bf16  512 0 b0", "m16 fp16  512 0 b0"):
    line = [l for l in lines if tag in l]
    assert len(line) == 1, lines
    assert "vgpr 256 agpr 256" in line[0] and "scratch    0 B" in line[0] and "mfma 256" in line[0], line
    assert "first..last MFMA: scratch ops 0, lane spills 0" in line[0], line
