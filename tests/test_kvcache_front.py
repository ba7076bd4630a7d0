"""The Python front end of the 16-bit KV-cache family — ffpa_attn_with_kvcache, _tree, _window, _softcap, _cascade and ffpa_attn_varlen_with_kvcache — answers
what tests/golden/kv_front_calls.json records, row by row and exactly: signature and docstring, type and full message of every refusal (single faults, and pairs
of faults that pin which check speaks first), and for every served call the ffpa_attn::* ops and hip.varlen_forward calls it makes with each argument's shape,
dtype, strides, device, value and IDENTITY with the caller's tensors, and the torch ops that make the boundaries and lengths it hands over (meta tensors under a
TorchDispatchMode: no GPU needed).  The list was recorded by tests/golden/make_kv_front_calls.py from the front end BEFORE its two checkers and its six steps
were folded into one of each.  Every row of the list is replayed; none is left out."""

import importlib.util
import os

import pytest

from conftest import ROOT

_GOLDEN = os.path.join(ROOT, "tests", "golden")
_spec = importlib.util.spec_from_file_location("make_kv_front_calls", os.path.join(_GOLDEN, "make_kv_front_calls.py"))
recorder = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(recorder)

RECORD = recorder.load()


def test_the_list_is_the_recorders_list():
  """Every row the recorder would take today is in the list and the list holds nothing else, so that "every row is replayed" means every row there is."""
  key = lambda r: sorted((k, str(v)) for k, v in r.items() if k != "want")
  want = [dict(func=f, layout=l, faults=x) for f, l, x in recorder.refusal_rows()]
  assert sorted(map(key, RECORD["refusals"])) == sorted(map(key, want))
  assert sorted(map(key, RECORD["served"])) == sorted(map(key, recorder.served_rows()))
  assert sorted(RECORD["signatures"]) == sorted(recorder.FUNCS)


def test_every_raise_is_reached_or_listed():
  """The recorder's own proof of coverage holds for the working tree: a single-fault row ends on every ``raise`` of the checked functions but the listed ones."""
  _, raises, unreachable = recorder.record()
  assert raises > unreachable == len(recorder.UNREACHABLE)


def test_signatures_and_docstrings_are_the_recorded_ones():
  assert recorder.signatures() == RECORD["signatures"]


@pytest.mark.parametrize("kind", ["refusals", "served"])
@pytest.mark.parametrize("func", recorder.FUNCS)
def test_rows_answer_what_was_recorded(func, kind):
  rows = [r for r in RECORD[kind] if r["func"] == func]
  assert len(rows) >= (190 if kind == "refusals" else 24), (func, kind)
  bad = []
  for row in rows:
    got = recorder.replay(kind, row)
    if got != row["want"]:
      bad.append(({k: v for k, v in row.items() if k != "want"}, got, row["want"]))
  assert not bad, f"{len(bad)} of {len(rows)} rows differ (row, got, recorded): {bad[:3]}"
