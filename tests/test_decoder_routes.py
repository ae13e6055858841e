"""The capability matrix of ``decoder.py``, replayed: ``tests/golden/decoder_routes.json`` holds, for every (mode, init_q, compute,
grad, hip_* flags) combination, where ``ImplicitDecoder.forward`` sends the call or the refusal it raises (part A), what each chunk
loop hands to the decode functions (part B) and what the functional entry points check and launch (part C), as
``tests/golden/make_decoder_routes.py`` recorded them.  The same recorder runs here against the code under test; every outcome
must be the recorded one.  CPU only: the kernels are stubs, the library's host functions are the real ones."""
import importlib.util
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def rec():
    spec = importlib.util.spec_from_file_location("make_decoder_routes", os.path.join(GOLDEN, "make_decoder_routes.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


@pytest.fixture(scope="module")
def golden(rec):
    with open(rec.PATH) as f:
        return json.load(f)


def _same(got, want, labels, what):
    assert len(got) == len(want), f"{what}: {len(got)} cases run, {len(want)} recorded"
    bad = [(label, g, w) for label, g, w in zip(labels, got, want) if g != w]
    lines = [f"{label}\n    now:      {g}\n    recorded: {w}" for label, g, w in bad[:8]]
    assert not bad, f"{what}: {len(bad)} of {len(got)} outcomes differ from the recording; the first:\n" + "\n".join(lines)


def test_forward_routes(rec, golden):
    """Part A: 5 modes x init_q x 4 computes x 128 flag settings x 5 call shapes, with and without the device check stubbed."""
    want = rec.expand(golden["A"])
    assert len(want) == 2 * 5 * 2 * 4 * 128 * 5
    _same(json.loads(json.dumps(rec.run_a())), want, rec.cases_a(), "forward")


def test_chunk_loops(rec, golden):
    """Part B: every loop takes more than one turn, and hands over these rows and these buffers."""
    want = rec.expand(golden["B"])
    assert all(o[0] == "calls" and len(o[1]) > 1 for o in want)
    _same(json.loads(json.dumps(rec.run_b())), want, rec.cases_b(), "chunk loops")


def test_entry_points(rec, golden):
    """Part C: one good call per launch entry point, one call per refusal in the bodies of the functional entry points."""
    want = golden["C"]
    launched = {call[0] for _, o in want if o[0] == "calls" for call in o[1]}
    assert launched == {"diinn_decode_ex", "diinn_decode_qonly_x3", "diinn_decode_mode4", "diinn_decode_mode4_x3",
                        "diinn_decode_initq", "diinn_decode_initq_x3", "diinn_decode_initq_mode1", "diinn_decode_initq_mode2",
                        "diinn_decode_initq_mode4", "diinn_decode_win", "diinn_decode_tile_win", "diinn_liif_decode",
                        "diinn_metasr_decode"}
    got = json.loads(json.dumps(rec.run_c()))
    _same([o for _, o in got], [o for _, o in want], [label for label, _ in got], "entry points")
    assert [label for label, _ in got] == [label for label, _ in want]
