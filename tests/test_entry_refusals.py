"""The decode entry points' argument checks, replayed: ``tests/golden/entry_refusals.json`` holds, for every check an entry point
makes in front of its first launch and for every pair of adjacent checks, the status it answers, as
``tests/golden/make_entry_refusals.py`` recorded them.  CPU only, and only refusals: the calls carry fake pointers that nothing
dereferences.  With a GPU visible the module skips itself -- its subject is host code, and a validation bug must not become a launch
on fake pointers there."""
import importlib.util
import json
import os

import pytest
import torch

if torch.cuda.is_available():
    pytest.skip("host-side validation only: runs where no GPU is visible", allow_module_level=True)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
REFUSALS = (1, 2, 4)            # DIINN_ERR_INVALID_ARG, _UNSUPPORTED, _TOO_LARGE


@pytest.fixture(scope="module")
def rec():
    spec = importlib.util.spec_from_file_location("make_entry_refusals", os.path.join(GOLDEN, "make_entry_refusals.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


@pytest.fixture(scope="module")
def golden(rec):
    with open(rec.PATH) as f:
        return json.load(f)


def test_the_recording_holds_refusals_only(rec, golden):
    """No stored row passed validation (0) or reached a HIP call (3); every entry point of the generator's table has rows, and
    the stored arguments are the ones the generator builds today."""
    assert golden and all(r["status"] in REFUSALS for r in golden)
    assert {r["fn"] for r in golden} == set(rec.ENTRIES)
    assert [(r["fn"], r["case"], r["args"]) for r in golden] == [(n, c, a) for n, c, a in rec.rows()]


def test_every_refusal_is_the_recorded_one(rec, golden):
    import diinn_amd._native as N
    lib = N.load()
    bad = []
    for r in golden:
        assert r["status"] in REFUSALS, r                       # (checked before the call: a 0 / 3 row is never replayed)
        got = rec.call(lib, r["fn"], r["args"])
        if got != r["status"]:
            bad.append(f"{r['fn']} [{r['case']}]: now {got}, recorded {r['status']}")
    assert not bad, f"{len(bad)} of {len(golden)} statuses differ from the recording; the first:\n" + "\n".join(bad[:12])


def test_regenerating_gives_the_same_bytes(rec):
    with open(rec.PATH) as f:
        assert rec.dumps(rec.record()) == f.read()
