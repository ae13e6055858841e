#!/usr/bin/env python3
"""The capability matrix of ``diinn_amd.decoder`` as a recording: which combination of (mode, init_q, compute, grad, hip_* flags) runs
where, which refuses with which message, what the chunk loops hand to the decode functions, and what the functional entry points
check before they launch.  Runs on the CPU in seconds (needs the built library for its host functions; no GPU, no reference).

  A  ``ImplicitDecoder.forward``: modes 1..5 x init_q x the four ``compute`` names x all 128 settings of the seven hip_* flags x
     five call shapes, once with ``decoder._require_cuda`` stubbed and once with the real one (a CPU tensor then raises "ROCm GPU"
     wherever the device is first looked at, which pins the position of that check among the refusals).  ``decode_features``,
     ``decode_features_initq`` and the five ``decode_with_grad`` functions are stubs that record what they were given.
  B  the chunk loops of ``forward`` at geometries where each takes more than one turn.
  C  ``decode_features``, ``decode_features_initq``, ``decode_window``, ``decode_tile``, ``liif_decode_features`` and
     ``metasr_decode_features`` on CPU tensors with every launch entry point of the library replaced by a recorder of its integer
     arguments: one good call per entry point they reach, one call per refusal in their bodies.

An outcome is ``["raise", type, message]`` or ``["calls", [...]]``.  A and B are stored as the list of distinct outcomes plus a
run-length coded index per case (``[outcome, run, outcome, run, ...]`` in the order of ``cases_a()`` / ``cases_b()``), C as one
labelled outcome per call.  ``tests/test_decoder_routes.py`` replays ``record()`` against the committed file.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_decoder_routes.py
"""
import contextlib
import itertools
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

PATH = os.path.join(HERE, "decoder_routes.json")
FLAGS = ("hip_autograd", "hip_autograd_mode4", "hip_initq_modes", "hip_initq_split_bf16", "hip_autograd_initq_modes",
         "hip_autograd_split_bf16", "hip_modes_split_bf16")
MODES = (1, 2, 3, 4, 5)
COMPUTES = ("f32", "bf16", "bf16_full", "bf16x3")
# (grad enabled, bsize, size)
CALLS = ((True, None, (8, 8)), (False, None, (8, 8)), (True, 30000, (8, 8)), (True, None, (1, 8)), (False, None, (1, 8)))
GRAD_MODULES = ("training", "initq_training", "mode4_training", "initq_modes_training", "split_training")
LAUNCH_PREFIXES = ("diinn_decode", "diinn_liif_decode", "diinn_metasr_decode")


def _numel(t):
    return None if t is None else int(t.numel())


def _rows(rows):
    return None if rows is None else [int(rows[0]), int(rows[1])]


class _Stream:
    cuda_stream = 0


@contextlib.contextmanager
def forward_stubs(log, require_cuda_stub=True):
    """The seams of parts A and B: everything ``forward`` hands its work to appends to ``log`` instead."""
    def decode_features(feat, packed, size, out=None, workspace=None, rows=None, sin_mode=N.SIN_DEFAULT, compute="f32", mode=3,
                        head=None, taps=None, initq=None, pix=None, initq_x3=None, modes_x3=False):
        log.append({"fn": "decode_features", "size": [int(v) for v in size], "mode": mode, "compute": compute, "rows": _rows(rows),
                    "modes_x3": bool(modes_x3), "sin_mode": int(sin_mode),
                    "images": [n for n, t in (("head", head), ("initq", initq), ("initq_x3", initq_x3)) if t is not None],
                    "workspace": _numel(workspace), "pix": _numel(pix), "taps": _numel(taps), "out": _numel(out)})
        return out if out is not None else torch.empty((feat.shape[0], 3, int(size[0]), int(size[1])))

    def decode_features_initq(feat, packed, initq, size, mode, head=None, taps=None, pix=None, rows=None, out=None,
                              sin_mode=N.SIN_DEFAULT, planes_rows=None):
        log.append({"fn": "decode_features_initq", "size": [int(v) for v in size], "mode": mode, "rows": _rows(rows),
                    "sin_mode": int(sin_mode), "planes_rows": planes_rows,
                    "images": [n for n, t in (("head", head), ("initq", initq)) if t is not None],
                    "pix": _numel(pix), "taps": _numel(taps), "out": _numel(out)})
        return out if out is not None else torch.empty((feat.shape[0], 3, int(size[0]), int(size[1])))

    def packed_weights(self, device):
        # the images the real one packs beside the body image, as tokens
        self._packed_head = "head" if self.mode == 4 else None
        self._packed_initq = "initq" if self.init_q else None
        self._packed_initq_x3 = "initq_x3" if self.init_q else None
        return "packed"

    def grad_stub(name):
        def decode_with_grad(dec, x, size):
            log.append({"fn": name + ".decode_with_grad", "size": [int(v) for v in size]})
            return torch.empty((x.shape[0], 3, int(size[0]), int(size[1])))
        return decode_with_grad

    with contextlib.ExitStack() as st:
        st.enter_context(mock.patch.object(D, "decode_features", decode_features))
        st.enter_context(mock.patch.object(D, "decode_features_initq", decode_features_initq))
        st.enter_context(mock.patch.object(D.ImplicitDecoder, "packed_weights", packed_weights))
        for name in GRAD_MODULES:
            module = __import__("diinn_amd." + name, fromlist=["decode_with_grad"])
            st.enter_context(mock.patch.object(module, "decode_with_grad", grad_stub(name)))
        st.enter_context(mock.patch.object(torch.cuda, "is_current_stream_capturing", lambda: False))
        st.enter_context(mock.patch.object(torch.cuda, "current_stream", lambda device=None: _Stream()))
        if require_cuda_stub:
            st.enter_context(mock.patch.object(D, "_require_cuda", lambda t, what: None))
        yield


def _outcome(fn, log):
    del log[:]
    try:
        fn()
    except Exception as e:  # noqa: BLE001  (the refusal IS the outcome)
        return ["raise", type(e).__name__, str(e)]
    return ["calls", [dict(c) if isinstance(c, dict) else c for c in log]]


def _configure(dec, compute, flags):
    dec.compute = compute
    for name, value in zip(FLAGS, flags):
        setattr(dec, name, value)
    for cache in (dec._workspaces, dec._tap_workspaces, dec._pix_workspaces):
        cache.clear()


def _forward(dec, x, grad, bsize, size):
    with (torch.enable_grad() if grad else torch.no_grad()):
        dec(x, list(size), bsize)


def cases_a():
    """Labels of part A's cases, in recording order."""
    for stub, mode, init_q, compute in itertools.product((True, False), MODES, (False, True), COMPUTES):
        for flags in itertools.product((False, True), repeat=len(FLAGS)):
            for grad, bsize, size in CALLS:
                yield {"require_cuda_stub": stub, "mode": mode, "init_q": init_q, "compute": compute,
                       "flags": [n for n, v in zip(FLAGS, flags) if v], "grad": grad, "bsize": bsize, "size": list(size)}


def run_a():
    """Part A: one outcome per case of ``cases_a()``."""
    x = torch.zeros(1, 64, 4, 4)
    decoders = {(m, q): D.ImplicitDecoder(mode=m, init_q=q) for m in MODES for q in (False, True)}
    log, outcomes = [], []
    for stub in (True, False):
        with forward_stubs(log, require_cuda_stub=stub):
            for mode, init_q, compute in itertools.product(MODES, (False, True), COMPUTES):
                dec = decoders[mode, init_q]
                for flags in itertools.product((False, True), repeat=len(FLAGS)):
                    for grad, bsize, size in CALLS:
                        _configure(dec, compute, flags)
                        outcomes.append(_outcome(lambda: _forward(dec, x, grad, bsize, size), log))
    return outcomes


# part B: (label, mode, init_q, compute, flags set, size, INITQ_CHUNK_BYTES or None)
_INITQ_CAP = 8 * 1 * 4 * 5120
LOOPS = (
    ("mode4 f32 300x2", 4, False, "f32", (), (300, 2), None),
    ("init_q mode3 f32 20x4", 3, True, "f32", (), (20, 4), _INITQ_CAP),
    ("init_q mode3 bf16x3 20x4", 3, True, "bf16x3", ("hip_initq_split_bf16",), (20, 4), _INITQ_CAP),
    ("init_q mode1 f32 20x4", 1, True, "f32", ("hip_initq_modes",), (20, 4), _INITQ_CAP),
    ("init_q mode2 f32 20x4", 2, True, "f32", ("hip_initq_modes",), (20, 4), _INITQ_CAP),
    ("init_q mode4 f32 20x4", 4, True, "f32", ("hip_initq_modes",), (20, 4), _INITQ_CAP),
    ("mode4 bf16x3 300x2", 4, False, "bf16x3", ("hip_modes_split_bf16",), (300, 2), None),
)


def cases_b():
    for loop in LOOPS:
        yield {"loop": loop[0]}


def run_b():
    """Part B: the calls of every chunk loop."""
    x = torch.zeros(1, 64, 4, 4)
    log, outcomes = [], []
    with forward_stubs(log):
        for _, mode, init_q, compute, on, size, cap in LOOPS:
            dec = D.ImplicitDecoder(mode=mode, init_q=init_q)
            _configure(dec, compute, [name in on for name in FLAGS])
            if cap is not None:
                dec.INITQ_CHUNK_BYTES = cap
            outcomes.append(_outcome(lambda: _forward(dec, x, False, None, size), log))
    return outcomes


class _LibProxy:
    """The real library with every launch entry point replaced by a recorder of (name, its integer arguments)."""

    def __init__(self, lib, log):
        self._lib, self._log = lib, log

    def __getattr__(self, name):
        if not name.startswith(LAUNCH_PREFIXES):
            return getattr(self._lib, name)

        def launch(*args):
            self._log.append([name, [a for a in args if isinstance(a, int)]])
            return 0
        return launch


@contextlib.contextmanager
def entry_stubs(log):
    """The seams of part C."""
    proxy = _LibProxy(N.load(), log)
    with contextlib.ExitStack() as st:
        st.enter_context(mock.patch.object(N, "load", lambda: proxy))
        st.enter_context(mock.patch.object(torch.cuda, "device", lambda device=None: contextlib.nullcontext()))
        st.enter_context(mock.patch.object(torch.cuda, "current_stream", lambda device=None: _Stream()))
        st.enter_context(mock.patch.object(D, "_require_cuda", lambda t, what: None))
        yield


def entry_calls():
    """Part C's calls: (label, thunk)."""
    f32, f64 = torch.float32, torch.float64
    feat, tok = torch.zeros(1, 64, 4, 4), torch.zeros(4)
    s = (8, 8)
    calls = []

    def add(label, fn, *args, **kw):
        calls.append((label, lambda: fn(*args, **kw)))

    df, dfi = D.decode_features, D.decode_features_initq
    # -- decode_features ---------------------------------------------------------------------------------------------------------
    for mode, compute, x3 in itertools.product((1, 2, 3, 4), COMPUTES, (False, True)):
        add(f"decode_features mode {mode} {compute} modes_x3={x3}", df, feat, tok, s, compute=compute, mode=mode, modes_x3=x3,
            head=tok if mode == 4 else None)
    add("decode_features mode 5", df, feat, tok, s, mode=5)
    add("decode_features band", df, feat, tok, s, rows=(2, 6))
    add("decode_features rows (3, 9) of 8", df, feat, tok, s, rows=(3, 9))
    add("decode_features feat dtype", df, feat.double(), tok, s)
    add("decode_features feat rank", df, feat[0], tok, s)
    add("decode_features feat channels", df, feat[:, :63], tok, s)
    add("decode_features size of length 3", df, feat, tok, (8, 8, 8))
    add("decode_features out given", df, feat, tok, s, out=torch.zeros(1, 3, 8, 8))
    add("decode_features out shape", df, feat, tok, s, out=torch.zeros(1, 3, 8, 7))
    add("decode_features out dtype", df, feat, tok, s, out=torch.zeros(1, 3, 8, 8, dtype=f64))
    add("decode_features out non-contiguous", df, feat, tok, s, out=torch.zeros(1, 3, 8, 16)[..., ::2])
    add("decode_features workspace given", df, feat, tok, s, workspace=torch.zeros(1 * 4 * 4 * 1024))
    add("decode_features workspace small", df, feat, tok, s, workspace=torch.zeros(1 * 4 * 4 * 1024 - 1))
    add("decode_features workspace fp64", df, feat, tok, s, workspace=torch.zeros(1 * 4 * 4 * 512, dtype=f64))
    add("decode_features workspace non-contiguous", df, feat, tok, s, workspace=torch.zeros(2 * 4 * 4 * 1024)[::2])
    add("decode_features mode 4 band", df, feat, tok, s, mode=4, head=tok, rows=(2, 6))
    add("decode_features mode 4 without head", df, feat, tok, s, mode=4)
    add("decode_features mode 4 at 1 x 8", df, feat, tok, (1, 8), mode=4, head=tok)
    add("decode_features mode 4 at 8 x 1", df, feat, tok, (8, 1), mode=4, head=tok)
    add("decode_features mode 4 rows (0, 9)", df, feat, tok, s, mode=4, head=tok, rows=(0, 9))
    add("decode_features mode 4 rows (-1, 4)", df, feat, tok, s, mode=4, head=tok, rows=(-1, 4))
    add("decode_features mode 4 rows (3, 9) of 8", df, feat, tok, s, mode=4, head=tok, rows=(3, 9))
    add("decode_features mode 4 taps given", df, feat, tok, s, mode=4, head=tok, taps=torch.zeros(1 << 16))
    add("decode_features mode 4 taps small", df, feat, tok, s, mode=4, head=tok, taps=torch.zeros(16))
    add("decode_features mode 4 taps non-contiguous", df, feat, tok, s, mode=4, head=tok, taps=torch.zeros(1 << 17)[::2])
    add("decode_features initq", df, feat, tok, s, initq=tok)
    add("decode_features initq band", df, feat, tok, s, initq=tok, rows=(2, 6))
    add("decode_features initq x3", df, feat, tok, s, initq=tok, initq_x3=tok, compute="bf16x3")
    add("decode_features initq mode 2", df, feat, tok, s, initq=tok, mode=2)
    add("decode_features initq bf16", df, feat, tok, s, initq=tok, compute="bf16")
    add("decode_features initq bf16x3 without initq_x3", df, feat, tok, s, initq=tok, compute="bf16x3")
    add("decode_features initq_x3 with bf16_full", df, feat, tok, s, initq=tok, initq_x3=tok, compute="bf16_full")
    add("decode_features initq_x3 without initq", df, feat, tok, s, initq_x3=tok, compute="bf16x3")
    add("decode_features initq_x3 with f32", df, feat, tok, s, initq=tok, initq_x3=tok)
    add("decode_features initq rows (0, 9)", df, feat, tok, s, initq=tok, rows=(0, 9))
    add("decode_features initq rows (-1, 4)", df, feat, tok, s, initq=tok, rows=(-1, 4))
    add("decode_features initq rows (3, 9) of 8", df, feat, tok, s, initq=tok, rows=(3, 9))
    add("decode_features initq rows (4, 4)", df, feat, tok, s, initq=tok, rows=(4, 4))
    add("decode_features initq pix given", df, feat, tok, s, initq=tok, pix=torch.zeros(1 * 8 * 8 * 1280))
    add("decode_features initq pix small", df, feat, tok, s, initq=tok, pix=torch.zeros(1 * 8 * 8 * 1280 - 1))
    add("decode_features initq pix fp64", df, feat, tok, s, initq=tok, pix=torch.zeros(1 * 8 * 8 * 1280, dtype=f64))
    add("decode_features initq out shape", df, feat, tok, s, initq=tok, out=torch.zeros(1, 3, 7, 8))
    add("decode_features initq feat dtype", df, feat.double(), tok, s, initq=tok)
    # -- decode_features_initq ---------------------------------------------------------------------------------------------------
    for mode in (1, 2, 4):
        head = tok if mode == 4 else None
        add(f"decode_features_initq mode {mode}", dfi, feat, tok, tok, s, mode, head=head)
        add(f"decode_features_initq mode {mode} band", dfi, feat, tok, tok, s, mode, head=head, rows=(2, 6))
        for planes_rows in (512, 1280):
            add(f"decode_features_initq mode {mode} planes_rows {planes_rows}", dfi, feat, tok, tok, s, mode, head=head,
                planes_rows=planes_rows)
        add(f"decode_features_initq mode {mode} rows (0, 9)", dfi, feat, tok, tok, s, mode, head=head, rows=(0, 9))
        add(f"decode_features_initq mode {mode} rows (-1, 4)", dfi, feat, tok, tok, s, mode, head=head, rows=(-1, 4))
        add(f"decode_features_initq mode {mode} rows (3, 9) of 8", dfi, feat, tok, tok, s, mode, head=head, rows=(3, 9))
        add(f"decode_features_initq mode {mode} pix small", dfi, feat, tok, tok, s, mode, head=head, pix=torch.zeros(64))
        add(f"decode_features_initq mode {mode} pix fp64", dfi, feat, tok, tok, s, mode, head=head,
            pix=torch.zeros(1 * 8 * 8 * 1280, dtype=f64))
    add("decode_features_initq mode 3", dfi, feat, tok, tok, s, 3)
    add("decode_features_initq mode 5", dfi, feat, tok, tok, s, 5)
    add("decode_features_initq mode 4 without head", dfi, feat, tok, tok, s, 4)
    add("decode_features_initq mode 4 at 1 x 8", dfi, feat, tok, tok, (1, 8), 4, head=tok)
    add("decode_features_initq mode 4 pix and taps given", dfi, feat, tok, tok, s, 4, head=tok, pix=torch.zeros(1 * 8 * 8 * 1280),
        taps=torch.zeros(1 << 16))
    add("decode_features_initq mode 4 taps small", dfi, feat, tok, tok, s, 4, head=tok, taps=torch.zeros(16))
    add("decode_features_initq feat dtype", dfi, feat.double(), tok, tok, s, 1)
    add("decode_features_initq feat rank", dfi, feat[0], tok, tok, s, 1)
    add("decode_features_initq feat channels", dfi, feat[:, :63], tok, tok, s, 1)
    add("decode_features_initq size of length 3", dfi, feat, tok, tok, (8, 8, 8), 1)
    add("decode_features_initq out shape", dfi, feat, tok, tok, s, 2, out=torch.zeros(1, 3, 8, 7))
    add("decode_features_initq out dtype", dfi, feat, tok, tok, s, 2, out=torch.zeros(1, 3, 8, 8, dtype=f64))
    add("decode_features_initq out non-contiguous", dfi, feat, tok, tok, s, 2, out=torch.zeros(1, 3, 8, 16)[..., ::2])
    # -- decode_window -----------------------------------------------------------------------------------------------------------
    dw = D.decode_window
    for mode in (1, 2, 3):
        add(f"decode_window mode {mode}", dw, feat, 0, 4, tok, s, (0, 8), mode=mode)
    for compute in COMPUTES[1:]:
        add(f"decode_window mode 3 {compute}", dw, feat, 0, 4, tok, s, (0, 8), compute=compute)
    add("decode_window band", dw, feat, 0, 4, tok, s, (2, 6))
    add("decode_window mode 4", dw, feat, 0, 4, tok, s, (0, 8), mode=4)
    add("decode_window mode 2 bf16", dw, feat, 0, 4, tok, s, (0, 8), mode=2, compute="bf16")
    add("decode_window feat_win dtype", dw, feat.double(), 0, 4, tok, s, (0, 8))
    add("decode_window feat_win channels", dw, feat[:, :63].contiguous(), 0, 4, tok, s, (0, 8))
    add("decode_window feat_win non-contiguous", dw, torch.zeros(1, 64, 4, 8)[..., ::2], 0, 4, tok, s, (0, 8))
    add("decode_window size of length 3", dw, feat, 0, 4, tok, (8, 8, 8), (0, 8))
    add("decode_window p_win given", dw, feat, 0, 4, tok, s, (0, 8), p_win=torch.zeros(1 * 4 * 4 * 1024))
    add("decode_window p_win small", dw, feat, 0, 4, tok, s, (0, 8), p_win=torch.zeros(1 * 4 * 4 * 1024 - 1))
    add("decode_window p_win fp64", dw, feat, 0, 4, tok, s, (0, 8), p_win=torch.zeros(1 * 4 * 4 * 1024, dtype=f64))
    add("decode_window out_win given", dw, feat, 0, 4, tok, s, (2, 6), out_win=torch.zeros(1, 3, 4, 8))
    add("decode_window out_win shape", dw, feat, 0, 4, tok, s, (2, 6), out_win=torch.zeros(1, 3, 8, 8))
    add("decode_window out_win dtype", dw, feat, 0, 4, tok, s, (2, 6), out_win=torch.zeros(1, 3, 4, 8, dtype=f64))
    # -- decode_tile -------------------------------------------------------------------------------------------------------------
    dt = D.decode_tile
    p_win = torch.zeros(1 * 4 * 4 * 1024)
    for mode in (1, 2, 3):
        add(f"decode_tile mode {mode}", dt, p_win, 0, (1, 4, 4), tok, s, (0, 8), (0, 8), torch.zeros(1, 3, 8, 8), mode=mode)
    add("decode_tile into a canvas", dt, p_win, 0, (1, 4, 4), tok, s, (2, 6), (1, 5), torch.zeros(1, 3, 9, 11)[:, :, 3:7, 2:6])
    add("decode_tile mode 3 bf16x3", dt, p_win, 0, (1, 4, 4), tok, s, (0, 8), (0, 8), torch.zeros(1, 3, 8, 8), compute="bf16x3")
    add("decode_tile non-unit x stride", dt, p_win, 0, (1, 4, 4), tok, s, (0, 8), (0, 8), torch.zeros(1, 3, 8, 16)[..., ::2])
    add("decode_tile one column of a strided view", dt, p_win, 0, (1, 4, 4), tok, s, (0, 8), (3, 4), torch.zeros(1, 3, 8, 2)[..., ::2])
    add("decode_tile out shape", dt, p_win, 0, (1, 4, 4), tok, s, (0, 8), (0, 8), torch.zeros(1, 3, 8, 7))
    add("decode_tile out dtype", dt, p_win, 0, (1, 4, 4), tok, s, (0, 8), (0, 8), torch.zeros(1, 3, 8, 8, dtype=f64))
    add("decode_tile p_win dtype", dt, p_win.double(), 0, (1, 4, 4), tok, s, (0, 8), (0, 8), torch.zeros(1, 3, 8, 8))
    add("decode_tile p_win size", dt, p_win[:-1], 0, (1, 4, 4), tok, s, (0, 8), (0, 8), torch.zeros(1, 3, 8, 8))
    add("decode_tile mode 4", dt, p_win, 0, (1, 4, 4), tok, s, (0, 8), (0, 8), torch.zeros(1, 3, 8, 8), mode=4)
    add("decode_tile mode 1 bf16", dt, p_win, 0, (1, 4, 4), tok, s, (0, 8), (0, 8), torch.zeros(1, 3, 8, 8), mode=1, compute="bf16")
    # -- the comparison decoders -------------------------------------------------------------------------------------------------
    for name, fn in (("liif_decode_features", D.liif_decode_features), ("metasr_decode_features", D.metasr_decode_features)):
        add(name, fn, feat, tok, s)
        add(f"{name} out and workspace given", fn, feat, tok, s, out=torch.zeros(1, 3, 8, 8), workspace=torch.zeros(1 << 16))
        add(f"{name} workspace small", fn, feat, tok, s, workspace=torch.zeros(16))
        add(f"{name} out shape", fn, feat, tok, s, out=torch.zeros(1, 3, 8, 7))
        add(f"{name} out dtype", fn, feat, tok, s, out=torch.zeros(1, 3, 8, 8, dtype=f64))
        add(f"{name} feat dtype", fn, feat.double(), tok, s)
        add(f"{name} feat rank", fn, feat[0], tok, s)
        add(f"{name} size of length 3", fn, feat, tok, (8, 8, 8))
    return calls


def run_c():
    """Part C: (label, outcome) per call of ``entry_calls()``."""
    log, outcomes = [], []
    with entry_stubs(log):
        for label, thunk in entry_calls():
            outcomes.append([label, _outcome(thunk, log)])
    return outcomes


def _compact(outcomes):
    """(distinct outcomes in order of first appearance, [outcome, run, outcome, run, ...])."""
    distinct, where, rle = [], {}, []
    for o in outcomes:
        key = json.dumps(o, sort_keys=True)
        if key not in where:
            where[key] = len(distinct)
            distinct.append(o)
        i = where[key]
        if rle and rle[-2] == i:
            rle[-1] += 1
        else:
            rle += [i, 1]
    return distinct, rle


def expand(part):
    """The per-case outcomes of a stored part A or B."""
    rle = part["index"]
    return [part["outcomes"][i] for i, run in zip(rle[0::2], rle[1::2]) for _ in range(run)]


def record():
    a, b = _compact(run_a()), _compact(run_b())
    return {"A": {"outcomes": a[0], "index": a[1]}, "B": {"outcomes": b[0], "index": b[1]}, "C": run_c()}


def dumps(rec) -> str:
    """One outcome per line, the indices on one line each: compact and still diffable."""
    def part(p):
        return ('{"outcomes":[\n' + ",\n".join(json.dumps(o, sort_keys=True, separators=(",", ":")) for o in p["outcomes"])
                + '\n],\n"index":' + json.dumps(p["index"], separators=(",", ":")) + "}")
    c = "[\n" + ",\n".join(json.dumps(o, sort_keys=True, separators=(",", ":")) for o in rec["C"]) + "\n]"
    return '{"A":' + part(rec["A"]) + ',\n"B":' + part(rec["B"]) + ',\n"C":' + c + "}\n"


def main():
    rec = record()
    text = dumps(rec)
    assert json.loads(text) == json.loads(json.dumps(rec)), "the compact form must read back as what was recorded"
    with open(PATH, "w") as f:
        f.write(text)
    n_a = sum(rec["A"]["index"][1::2])
    print(f"part A: {n_a} cases, {len(rec['A']['outcomes'])} distinct outcomes;  part B: {len(rec['B']['outcomes'])} loops;  "
          f"part C: {len(rec['C'])} calls")
    print("wrote", PATH, os.path.getsize(PATH), "bytes")


if __name__ == "__main__":
    main()
