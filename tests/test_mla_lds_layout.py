"""Host replay of the SHARED latent-tile image of the MLA build (tools/sim_lds_layout.py ``check_m16_shared``; csrc/ffpa_fwd_m16_tile.inc under FFPA_M16_MLA_ON):
at D = 576 one source-side swizzle has to serve the ds_read_b128 K-fragment groups AND the ds_read_b64_tr_b16 halves of the V^T fragments, both of which read
the image the LDS-DMA wrote once.  The counts DESIGN section 15 quotes are pinned here; the simulator is the evidence (nobody has measured
SQ_LDS_BANK_CONFLICT for this image)."""
import importlib.util
import os

_spec = importlib.util.spec_from_file_location(
    "sim_lds_layout", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "sim_lds_layout.py"))
sim = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(sim)


def test_the_kernels_map_is_conflict_free_for_both_read_patterns():
  assert sim.check_m16_shared(576) == (1, 1, 0, 0)
  assert sim.mla_sw(576, 13) == sim.m16_v_sw(576, 13)  # (the V map of the 16x16x32 build)


def test_the_candidates_design_quotes():
  """The K map costs every transpose-read half a 2-way conflict (2 waves x 18 column blocks x 2 reads x 2 halves = 144 extra cycles per tile); no swizzle costs
  both patterns 4 ways; the V map is free for both."""
  got = {name: sim.check_m16_shared(576, fn, quiet=True) for name, fn in sim.MLA_CANDIDATES.items()}
  assert got == {"k map": (1, 2, 0, 144), "v map": (1, 1, 0, 0), "none": (4, 4, 432, 432)}


def test_the_existing_layouts_report_what_they_reported():
  assert sim.check_m16(576) == (1, 1) and sim.check(576, 2) == (1, 1)
