#!/usr/bin/env python3
"""The kernel launches of the training paths as a recording: which entry points of the library a whole autograd Function enqueues,
in which order and with which integer arguments.  Runs on the CPU in seconds (needs the built library for its host functions; no
GPU, no reference).

Every stream-taking entry point of the library is replaced by a recorder of (name, its integer arguments); ``torch.cuda.device`` and
``torch.cuda.current_stream`` are stubs and ``torch.Tensor.is_cuda`` answers true, so ``Function.apply(...).sum().backward()`` runs
through on CPU tensors: the Python of the forward and of the backward is the code under test, the numbers it moves are not.
Pointer arguments are not recorded (the GPU suite's gradient tests cover what the kernels are handed).

  cases   mode 3, modes 1 and 2, mode 4, split-bf16 mode 3, init_q mode 3, init_q modes 1 / 2 / 4, LIIF and MetaSR, each at
          B=1, 3x2 -> 9x4 (36 pixels and 6 cells: both last tiles ragged) and B=2, 4x4 -> 8x8 (128 pixels, 32 cells: whole tiles), each
          with and without a gradient for the features; LIIF with ``layers.0.weight`` frozen, MetaSR with ``layers.2.*`` frozen.

``tests/test_training_launches.py`` replays ``record()`` against the committed file.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_training_launches.py
"""
import contextlib
import ctypes as C
import json
import os
import sys
from unittest import mock

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

import diinn_amd._native as N  # noqa: E402
import diinn_amd.decoder as D  # noqa: E402
import diinn_amd.initq_modes_training as IM  # noqa: E402
import diinn_amd.initq_training as IQ  # noqa: E402
import diinn_amd.liif_training as LT  # noqa: E402
import diinn_amd.metasr_training as MT  # noqa: E402
import diinn_amd.mode4_training as M4  # noqa: E402
import diinn_amd.split_training as ST  # noqa: E402
import diinn_amd.training as T  # noqa: E402

PATH = os.path.join(HERE, "training_launches.json")
SHAPES = ((1, 3, 2, 9, 4), (2, 4, 4, 8, 8))          # (B, H, W, Hu, Wu)
SIN_MODE = N.SIN_DEFAULT


def takes_stream(name: str) -> bool:
    """An entry point whose first argument is the stream (include/diinn_hip.h: every ``void*`` first argument is one)."""
    return N.SIGNATURES[name][1][:1] == [C.c_void_p]


class _Stream:
    cuda_stream = 0


class _LibProxy:
    """The real library with every stream-taking entry point replaced by a recorder of (name, its integer arguments)."""

    def __init__(self, lib, log):
        self._lib, self._log = lib, log

    def __getattr__(self, name):
        if name not in N.SIGNATURES or not takes_stream(name):
            return getattr(self._lib, name)

        def launch(*args):
            self._log.append([name, [a for a in args if isinstance(a, int)]])
            return 0
        return launch


@contextlib.contextmanager
def stubs(log):
    proxy = _LibProxy(N.load(), log)
    with contextlib.ExitStack() as st:
        st.enter_context(mock.patch.object(N, "load", lambda: proxy))
        st.enter_context(mock.patch.object(torch.cuda, "device", lambda device=None: contextlib.nullcontext()))
        st.enter_context(mock.patch.object(torch.cuda, "current_stream", lambda device=None: _Stream()))
        st.enter_context(mock.patch.object(torch.cuda, "is_current_stream_capturing", lambda: False))
        st.enter_context(mock.patch.object(torch.Tensor, "is_cuda", property(lambda self: True)))
        st.enter_context(mock.patch.object(D, "_require_cuda", lambda t, what: None))
        yield


def _tensors(names, shapes, seed):
    gen = torch.Generator().manual_seed(seed)
    return [(torch.randn(shapes[name], generator=gen) * 0.05) for name in names]


# (label, Function, the integers between the sizes and the parameters, parameter names, parameter shapes)
FUNCTIONS = (
    ("mode 3", T.DecodeMode3Function, (SIN_MODE,), T.PARAM_NAMES, T.PARAM_SHAPES),
    ("mode 1", T.DecodeModes12Function, (SIN_MODE, 1), T.PARAM_NAMES, T.param_shapes(1)),
    ("mode 2", T.DecodeModes12Function, (SIN_MODE, 2), T.PARAM_NAMES, T.param_shapes(2)),
    ("mode 4", M4.DecodeMode4Function, (SIN_MODE,), T.PARAM_NAMES, T.param_shapes(4)),
    ("mode 3 split bf16", ST.DecodeMode3SplitFunction, (SIN_MODE,), T.PARAM_NAMES, T.PARAM_SHAPES),
    ("init_q mode 3", IQ.DecodeInitqFunction, (SIN_MODE,), IQ.INITQ_PARAM_NAMES, IQ.INITQ_PARAM_SHAPES),
    ("init_q mode 1", IM.DecodeInitqModesFunction, (SIN_MODE, 1), IQ.INITQ_PARAM_NAMES, IM.param_shapes(1)),
    ("init_q mode 2", IM.DecodeInitqModesFunction, (SIN_MODE, 2), IQ.INITQ_PARAM_NAMES, IM.param_shapes(2)),
    ("init_q mode 4", IM.DecodeInitqModesFunction, (SIN_MODE, 4), IQ.INITQ_PARAM_NAMES, IM.param_shapes(4)),
    ("LIIF", LT.LIIFFunction, (), LT.PARAM_NAMES, LT.PARAM_SHAPES),
    ("MetaSR", MT.MetaSRFunction, (), MT.PARAM_NAMES, MT.PARAM_SHAPES),
)
FROZEN = {"LIIF": ("layers.0.weight",), "MetaSR": ("layers.2.weight", "layers.2.bias")}


def cases():
    """(label, Function, extra integers, names, shapes, (B, H, W, Hu, Wu), feat requires grad, frozen names) in recording order."""
    for label, fn, extra, names, shapes in FUNCTIONS:
        for shape in SHAPES:
            dims = "B=%d %dx%d -> %dx%d" % shape
            yield f"{label}, {dims}", fn, extra, names, shapes, shape, True, ()
            yield f"{label}, {dims}, feat without grad", fn, extra, names, shapes, shape, False, ()
        if label in FROZEN:
            dims = "B=%d %dx%d -> %dx%d" % SHAPES[0]
            yield f"{label}, {dims}, {' and '.join(FROZEN[label])} frozen", fn, extra, names, shapes, SHAPES[0], True, FROZEN[label]


def run_case(fn, extra, names, shapes, shape, feat_grad, frozen, log):
    """One forward and backward of ``fn`` on fresh CPU tensors; returns the launches it made."""
    b, h, w, hu, wu = shape
    del log[:]
    feat = torch.randn(b, 64, h, w, generator=torch.Generator().manual_seed(7)).requires_grad_(feat_grad)
    params = [p.requires_grad_(name not in frozen) for name, p in zip(names, _tensors(names, shapes, 11))]
    fn.apply(feat, hu, wu, *extra, *params).sum().backward()
    return [list(call) for call in log]


def record():
    """[[label, [[entry point, [integers]], ...]], ...] over ``cases()``."""
    log, out = [], []
    with stubs(log):
        for label, *case in cases():
            out.append([label, run_case(*case, log)])
    return out


def dumps(rec) -> str:
    """One launch per line under its case's label."""
    blocks = []
    for label, calls in rec:
        lines = ",\n".join("  " + json.dumps(c, separators=(",", ":")) for c in calls)
        blocks.append("[" + json.dumps(label) + ",[\n" + lines + "\n]]")
    return "[\n" + ",\n".join(blocks) + "\n]\n"


def main():
    rec = record()
    text = dumps(rec)
    assert json.loads(text) == json.loads(json.dumps(rec)), "the compact form must read back as what was recorded"
    with open(PATH, "w") as f:
        f.write(text)
    for label, calls in rec:
        print(f"{len(calls):3d} launches  {label}")
    print("wrote", PATH, os.path.getsize(PATH), "bytes")


if __name__ == "__main__":
    main()
