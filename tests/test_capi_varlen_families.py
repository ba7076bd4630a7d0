"""The packed call and its eleven relatives (paged, tree, window, soft-cap and the seven latent calls: MLA, MLA tree, sparse, and over pools counted in bytes MLA
FP8, MLA tree FP8, sparse FP8, sparse over 656-byte rows) answer what tests/golden/capi_varlen_calls.json records,
call by call and exactly: status and message of *_plan, the plan, the *_kernel string, *_workspace_bytes, *_compact_slots, and status and message of the
launch export for everything it refuses before it touches the device (no GPU needed).  The list was recorded by tests/golden/make_capi_varlen_calls.py from the
library BEFORE the host layer was rewritten around one call descriptor and one plan per call: order and wording of every refusal are pinned to that.  The four forms
over byte pools were recorded later, from the library before the seven latent families became one planner over a variant's traits; for each of them the list holds one
refusal per step of that planner's order and, for every two steps that follow each other, one call that breaks both (the earlier step answers).

One answer is not the recorded library's: *_workspace_bytes of the packed, paged and tree calls for arguments their plan refuses.  Those three sized a launch that
the launch itself refuses (a bad pool, a bad mask); the list holds the contract instead, 0, which is what the other families always answered there."""

import importlib.util
import os

import pytest

from conftest import ROOT
from ffpa_attn_amd import hip

_GOLDEN = os.path.join(ROOT, "tests", "golden")
_spec = importlib.util.spec_from_file_location("make_capi_varlen_calls", os.path.join(_GOLDEN, "make_capi_varlen_calls.py"))
recorder = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(recorder)

CALLS = recorder.load()  # [(line, call, what was recorded for it)]
FORMS = sorted(recorder.FORMS)


@pytest.fixture(scope="module")
def lib():
  if not hip.library_available():
    from ffpa_attn_amd import build

    build.build()
  return hip.load_library()


def test_the_list_covers_every_form_both_ways():
  for form in FORMS:
    mine = [want for _, call, want in CALLS if call["form"] == form]
    assert sum(1 for g in mine if g["plan"][0] == 0) >= 20, form
    assert sum(1 for g in mine if g["plan"][0] != 0) >= 10, form
    assert sum(1 for g in mine if g["launch"][0] not in (0, recorder.ERR_NO_DEVICE)) >= 20, form


@pytest.mark.parametrize("form", FORMS)
def test_calls_answer_what_was_recorded(lib, form):
  import torch

  gpu = torch.cuda.is_available()
  bad = []
  for line, call, want in CALLS:
    if call["form"] != form:
      continue
    want = dict(want)
    # an accepted call's launch export stops at "no device" only where there is none: with a GPU it would launch on the made-up addresses
    launch = not (gpu and want["launch"][0] == recorder.ERR_NO_DEVICE)
    if not launch:
      del want["launch"]
    got = recorder.replay(lib, call, launch=launch)
    if got != want:
      bad.append((f"line {line}", {k: (got[k], want[k]) for k in want if got[k] != want[k]}))
  assert not bad, f"{len(bad)} calls differ (got, recorded): {bad[:5]}"
