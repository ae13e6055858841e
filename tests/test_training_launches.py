"""The kernel launches of the training paths, replayed: ``tests/golden/training_launches.json`` holds, for every autograd Function
of the package at two shapes, the entry points a forward and backward enqueue, in order, with their integer arguments, as
``tests/golden/make_training_launches.py`` recorded them.  The same recorder runs here against the code under test; every trace must
be the recorded one.  Under the same stubs: the rule of the weight-image caches ("kept while no parameter has changed").
CPU only: the kernels are stubs, the library's host functions are the real ones."""
import importlib.util
import json
import os

import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def rec():
    spec = importlib.util.spec_from_file_location("make_training_launches", os.path.join(GOLDEN, "make_training_launches.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


@pytest.fixture(scope="module")
def golden(rec):
    with open(rec.PATH) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def now(rec):
    """The recorder run once against the code under test."""
    return rec.record()


def test_recorded_cases(rec, golden):
    """The recording holds every case of the recorder, the launch counts the traces are known by, and these entry points."""
    assert [label for label, _ in golden] == [case[0] for case in rec.cases()]
    assert len(golden) == 11 * 4 + 2
    counts = {label: len(calls) for label, calls in golden}
    at = ", B=1 3x2 -> 9x4"
    assert (counts["mode 3" + at], counts["mode 4" + at], counts["init_q mode 3" + at], counts["LIIF" + at], counts["MetaSR" + at]) \
        == (16, 23, 23, 15, 8)
    assert {call[0] for _, calls in golden for call in calls} == {
        "diinn_precompute_P_wpu", "diinn_decode_train_fwd", "diinn_decode_train_fwd_qonly", "diinn_decode_train_fwd_x3",
        "diinn_cell_chain", "diinn_cell_chain_bwd", "diinn_pack_split_train", "diinn_head3x3_from_planes",
        "diinn_backward_data", "diinn_backward_data_qonly", "diinn_backward_data_x3", "diinn_backward_data_head3x3",
        "diinn_plane_gemm_nt", "diinn_plane_rowdot", "diinn_sum_parts", "diinn_backward_cell_sum", "diinn_unfold_tiled",
        "diinn_conv_ksplit", "diinn_decode_initq_train_fwd", "diinn_decode_initq_train_fwd_qonly", "diinn_initq_backward",
        "diinn_pixel_chain_bwd", "diinn_cell_sum_rows", "diinn_fold3x3", "diinn_liif_train_fwd", "diinn_liif_backward_data",
        "diinn_liif_cell_sum", "diinn_metasr_decode", "diinn_metasr_backward_cells"}


def test_training_launches(now, golden):
    """Every Function's forward and backward enqueue the recorded entry points, in the recorded order, with the recorded integers."""
    got = json.loads(json.dumps(now))
    assert [label for label, _ in got] == [label for label, _ in golden]
    bad = []
    for (label, calls), (_, want) in zip(got, golden):
        if calls != want:
            at = next((i for i, (a, b) in enumerate(zip(calls, want)) if a != b), min(len(calls), len(want)))
            bad.append(f"{label}: {len(calls)} launches now, {len(want)} recorded; first difference at launch {at}\n"
                       f"    now:      {calls[at] if at < len(calls) else None}\n    recorded: {want[at] if at < len(want) else None}")
    assert not bad, f"{len(bad)} of {len(got)} traces differ from the recording:\n" + "\n".join(bad[:8])


def test_recording_regenerates_byte_for_byte(rec, now):
    with open(rec.PATH) as f:
        assert rec.dumps(now) == f.read()


# ---------------------------------------------------------------------------
# the weight-image caches: one image per set of weights, kept while no parameter has been modified
# ---------------------------------------------------------------------------
def _image_functions(rec):
    """(id, the public image function of one training path as params -> image(s), parameter names, parameter shapes)."""
    T, M4, ST, IQ, IM, LT, MT = rec.T, rec.M4, rec.ST, rec.IQ, rec.IM, rec.LT, rec.MT
    return {
        "training.pack_on_device": (lambda p: T.pack_on_device(p, 3), T.PARAM_NAMES, T.PARAM_SHAPES),
        "split_training.pack_split_on_device": (ST.pack_split_on_device, T.PARAM_NAMES, T.PARAM_SHAPES),
        "mode4_training.images_on_device": (M4.images_on_device, T.PARAM_NAMES, T.param_shapes(4)),
        "initq_training.images_on_device": (IQ.images_on_device, IQ.INITQ_PARAM_NAMES, IQ.INITQ_PARAM_SHAPES),
        "initq_modes_training.images_on_device": (lambda p: IM.images_on_device(p, 4), IQ.INITQ_PARAM_NAMES, IM.param_shapes(4)),
        "liif_training.image_on_device": (LT.image_on_device, LT.PARAM_NAMES, LT.PARAM_SHAPES),
        "metasr_training.images_on_device": (MT.images_on_device, MT.PARAM_NAMES, MT.PARAM_SHAPES),
    }


def _same(a, b) -> bool:
    """The same object(s): an image function returns one tensor or a tuple of them."""
    if isinstance(a, torch.Tensor):
        return a is b
    return len(a) == len(b) and all(x is y for x, y in zip(a, b))


@pytest.mark.parametrize("which", ["training.pack_on_device", "split_training.pack_split_on_device", "mode4_training.images_on_device",
                                   "initq_training.images_on_device", "initq_modes_training.images_on_device",
                                   "liif_training.image_on_device", "metasr_training.images_on_device"])
def test_images_are_kept_while_no_parameter_has_changed(rec, which):
    """A repeated call answers the same object; an in-place update of the first or of the last parameter, and a second set of
    equal-shaped tensors, each give a new one (of a pair or triple: at least one new member -- mode 4 keeps the body image when
    only the head's tensors changed, and the head image when only the body's did)."""
    fn, names, shapes = _image_functions(rec)[which]
    with rec.stubs([]):
        params = rec._tensors(names, shapes, 3)
        first = fn(params)
        assert _same(fn(params), first)
        params[0].add_(1.0)
        second = fn(params)
        assert not _same(second, first)
        assert _same(fn(params), second)
        params[-1].mul_(2.0)
        third = fn(params)
        assert not _same(third, second)
        assert _same(fn(params), third)
        other = rec._tensors(names, shapes, 3)
        fourth = fn(other)
        assert not _same(fourth, third)
        assert _same(fn(other), fourth)
        assert not _same(fn(params), fourth)
