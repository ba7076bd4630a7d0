"""The two KV-cache append exports of the C-ABI — ffpa_attn_kvcache_append and ffpa_attn_kvcache_append_varlen — answer what
tests/golden/capi_append_calls.json records, call by call and exactly: status and ffpa_attn_last_error() of every refusal — each check of both exports broken
once, with and without a ``ffpa_paged_kv``, and for every two checks that follow each other one call that breaks both (the earlier one answers) — and NO_DEVICE
for the calls that pass every check (no GPU needed).  The list was recorded by tests/golden/make_capi_append_calls.py from the library BEFORE the two exports'
shared checks and their filling of the kernel's arguments were moved into helpers: order and wording of every refusal are pinned to that."""

import importlib.util
import os

import pytest

from conftest import ROOT
from ffpa_attn_amd import hip

_GOLDEN = os.path.join(ROOT, "tests", "golden")
_spec = importlib.util.spec_from_file_location("make_capi_append_calls", os.path.join(_GOLDEN, "make_capi_append_calls.py"))
recorder = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(recorder)

CALLS = recorder.load()


@pytest.fixture(scope="module")
def lib():
  if not hip.library_available():
    from ffpa_attn_amd import build

    build.build()
  return hip.load_library()


def test_the_list_is_the_recorders_list():
  key = lambda c: sorted((k, str(v)) for k, v in c.items() if k != "got")
  assert sorted(map(key, CALLS)) == sorted(map(key, recorder.calls()))
  for export in recorder.EXPORTS:
    for paged in (False, True):
      mine = [c["got"] for c in CALLS if c["export"] == export and c["paged"] == paged]
      assert sum(g == recorder.NO_DEVICE for g in mine) >= 8 and len({g[1] for g in mine}) >= 30, (export, paged)


@pytest.mark.parametrize("export", sorted(recorder.EXPORTS))
def test_calls_answer_what_was_recorded(lib, export):
  import torch

  gpu = torch.cuda.is_available()
  bad = []
  for call in CALLS:
    # an accepted call stops at "no device" only where there is none: with a GPU it would launch on the made-up addresses
    if call["export"] != export or (gpu and call["got"] == recorder.NO_DEVICE):
      continue
    got = recorder.replay(lib, call)
    if got != call["got"]:
      bad.append((call["paged"], call["why"], got, call["got"]))
  assert not bad, f"{len(bad)} calls differ (got, recorded): {bad[:5]}"
