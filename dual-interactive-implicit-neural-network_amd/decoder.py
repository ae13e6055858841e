"""Host side of the MI355X DIINN decode path: the reference's ``ImplicitDecoder``
interface, executed by the gfx950 kernels in libdiinn_hip.so.

Mirrors /root/reference/src/models/components/diinn.py:
  * ``ImplicitDecoder(in_channels=64, hidden_dims=[256]*4, mode=1, init_q=False)``
    registers parameters under the same names and shapes as diinn.py:40-92
    (``K.{i}.0.weight`` ..., ``Q.{i}.0.*``, ``last_layer.*``) so reference
    checkpoints ``load_state_dict`` unchanged;
  * ``forward(x, size, bsize=None)`` has the argument meaning of diinn.py:163-173.

The compute is the HIP path and only the HIP path: CPU tensors, a missing
library or decoder variants the kernels do not cover raise instead of silently
falling back.  PyTorch is used for device memory and the stream; under autograd
(training, modes 1-3, fp32) the forward is the HIP kernel with saved activations and the
backward is library GEMMs over those (training.py).
"""
from __future__ import annotations

import ctypes as C
import importlib
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn as nn

from . import _native
# the formula sheets live in sheets.py; tests, tools and the documents cite them under this module's name
from .sheets import (HIDDEN, INV_2PI_F32, P_CHANNELS, axis_tables, initq_forward_reference,  # noqa: F401
                     initq_modes_forward_reference, initq_modes_x3_forward_reference, initq_planes_reference, liif_x3_forward_reference,
                     modes_x3_forward_reference)

IN_CHANNELS = 64


class SineAct(nn.Module):
    """sin activation of the synthesis branch (reference: diinn.py:21-26)."""

    def forward(self, x):
        return torch.sin(x)


# ---------------------------------------------------------------------------
# packed weights
# ---------------------------------------------------------------------------
def _host_array(sd, prefix: str, name: str, shape) -> np.ndarray:
    """``sd[prefix + name]`` (a tensor or an array) as a contiguous fp32 host array of ``shape``."""
    t = sd[prefix + name]
    a = t.detach().to("cpu", torch.float32).numpy() if isinstance(t, torch.Tensor) else np.asarray(t, np.float32)
    return np.ascontiguousarray(a.reshape(shape), dtype=np.float32)


def pack_state_dict(sd, prefix: str = "", mode: int = 3) -> torch.Tensor:
    """Reference-named decoder tensors -> packed host image (1-D fp32 CPU tensor).

    ``sd`` maps ``{prefix}K.0.0.weight`` ... to tensors/arrays in the layouts of
    SURVEY.md App. A.1 (init_q=False).  Modes 2 and 3 share the layout (K.i is [256, 832]: 256
    chained inputs, then the 576 unfolded features); mode 1's K.i is [256, 256] (no feature
    columns, diinn.py:53-60) and is widened with zero feature columns, so P_i = bK_i for i >= 1.
    Mode 4 gives the BODY image: the mode-3 image of the same K / Q tensors with a zero 1x1 head; its 3x3 head is a
    second image (``pack_head3x3``).  Calls the C ABI ``diinn_pack_weights`` (include/diinn_hip.h)."""
    lib = _native.load()

    k0w = _host_array(sd, prefix, "K.0.0.weight", (HIDDEN, 576)); k0b = _host_array(sd, prefix, "K.0.0.bias", (HIDDEN,))
    if mode == 1:
        kw = []
        for i in (1, 2, 3):
            wide = np.zeros((HIDDEN, HIDDEN + 576), np.float32)
            wide[:, :HIDDEN] = _host_array(sd, prefix, f"K.{i}.0.weight", (HIDDEN, HIDDEN))
            kw.append(wide)
    else:
        kw = [_host_array(sd, prefix, f"K.{i}.0.weight", (HIDDEN, HIDDEN + 576)) for i in (1, 2, 3)]
    kb = [_host_array(sd, prefix, f"K.{i}.0.bias", (HIDDEN,)) for i in (1, 2, 3)]
    q0w = _host_array(sd, prefix, "Q.0.0.weight", (HIDDEN, 3)); q0b = _host_array(sd, prefix, "Q.0.0.bias", (HIDDEN,))
    qw = [_host_array(sd, prefix, f"Q.{i}.0.weight", (HIDDEN, HIDDEN)) for i in (1, 2, 3)]
    qb = [_host_array(sd, prefix, f"Q.{i}.0.bias", (HIDDEN,)) for i in (1, 2, 3)]
    if mode == 4:
        lw = np.zeros((3, HIDDEN), np.float32); lb = np.zeros((3,), np.float32)
    else:
        lw = _host_array(sd, prefix, "last_layer.weight", (3, HIDDEN)); lb = _host_array(sd, prefix, "last_layer.bias", (3,))

    packed = np.empty(lib.diinn_packed_weight_floats(), dtype=np.float32)
    f3 = _native._f3
    st = lib.diinn_pack_weights(
        _native.fptr(k0w), _native.fptr(k0b),
        f3(*[_native.fptr(a) for a in kw]), f3(*[_native.fptr(a) for a in kb]),
        _native.fptr(q0w), _native.fptr(q0b),
        f3(*[_native.fptr(a) for a in qw]), f3(*[_native.fptr(a) for a in qb]),
        _native.fptr(lw), _native.fptr(lb), _native.fptr(packed))
    _native.check(st, "diinn_pack_weights")
    return torch.from_numpy(packed)


def pack_head3x3(sd, prefix: str = "") -> torch.Tensor:
    """Mode 4's head, ``last_layer.weight`` [3,256,3,3] and ``last_layer.bias`` [3] (diinn.py:89-90), -> its packed host
    image (1-D fp32 CPU tensor; C ABI ``diinn_pack_head3x3``: [27][256] with row 3 (3 ky + kx) + c, the bias, a validity
    word)."""
    lib = _native.load()

    lw = _host_array(sd, prefix, "last_layer.weight", (3, HIDDEN, 3, 3)); lb = _host_array(sd, prefix, "last_layer.bias", (3,))
    packed = np.empty(lib.diinn_head3x3_packed_floats(), dtype=np.float32)
    _native.check(lib.diinn_pack_head3x3(_native.fptr(lw), _native.fptr(lb), _native.fptr(packed)), "diinn_pack_head3x3")
    return torch.from_numpy(packed)


def pack_initq(sd, prefix: str = "") -> torch.Tensor:
    """``init_q=True``: ``first_layer.0.weight`` [576,3,1,1], ``first_layer.0.bias`` [576], ``Q.0.0.weight`` [256,576,1,1] and
    ``Q.0.0.bias`` [256] (diinn.py:48-51,61-62) -> the init_q host image (1-D fp32 CPU tensor; C ABI ``diinn_pack_initq``:
    the first layer as [4][576], Q.0 as MFMA A operands in the piece order of the hoisted conv, its bias, a validity word;
    everything divided by 2 pi).  The body image of such a decoder is ``pack_state_dict`` of the same tensors with a zero
    [256,3] in place of ``Q.0.0.weight`` (``initq_body_state_dict``)."""
    lib = _native.load()

    fw, fb = _host_array(sd, prefix, "first_layer.0.weight", (576, 3)), _host_array(sd, prefix, "first_layer.0.bias", (576,))
    q0w, q0b = _host_array(sd, prefix, "Q.0.0.weight", (HIDDEN, 576)), _host_array(sd, prefix, "Q.0.0.bias", (HIDDEN,))
    packed = np.empty(lib.diinn_initq_packed_floats(), dtype=np.float32)
    _native.check(lib.diinn_pack_initq(_native.fptr(fw), _native.fptr(fb), _native.fptr(q0w), _native.fptr(q0b),
                                       _native.fptr(packed)), "diinn_pack_initq")
    return torch.from_numpy(packed)


def pack_initq_x3(sd, prefix: str = "") -> torch.Tensor:
    """``init_q=True`` in split-bf16 arithmetic: ``Q.0.0.weight`` [256,576,1,1] and ``Q.0.0.bias`` [256] -> the init_q SPLIT image
    (1-D fp32 CPU tensor; C ABI ``diinn_pack_initq_x3``: Q.0 / (2 pi) as hi / lo bf16 A operands in the piece order of the body
    image's section WPX, its bias / (2 pi), a validity word).  The third image of such a decode, beside ``pack_state_dict`` of
    ``initq_body_state_dict`` and ``pack_initq``."""
    lib = _native.load()
    q0w, q0b = _host_array(sd, prefix, "Q.0.0.weight", (HIDDEN, 576)), _host_array(sd, prefix, "Q.0.0.bias", (HIDDEN,))
    packed = np.empty(lib.diinn_initq_x3_packed_floats(), dtype=np.float32)
    _native.check(lib.diinn_pack_initq_x3(_native.fptr(q0w), _native.fptr(q0b), _native.fptr(packed)), "diinn_pack_initq_x3")
    return torch.from_numpy(packed)


def initq_body_state_dict(sd, prefix: str = ""):
    """The tensors ``pack_state_dict(..., mode=3)`` takes for an ``init_q=True`` decoder: the same dict with a zero [256,3]
    in place of the 576-wide ``Q.0.0.weight`` (the init_q kernels never read the body image's Q0 rows)."""
    body = dict(sd)
    body[prefix + "Q.0.0.weight"] = np.zeros((HIDDEN, 3), np.float32)
    return body


def initq_chunk_rows(b: int, wu: int, cap_bytes: int) -> int:
    """HR rows per chunk of the init_q decode: the largest multiple of 8 (``decode_kernel``'s block rows) whose pixel planes,
    ``b * rows * wu * 5120`` bytes, stay within ``cap_bytes``; at least 8."""
    per_row = int(b) * int(wu) * (P_CHANNELS + HIDDEN) * 4
    return max(8, (int(cap_bytes) // per_row) // 8 * 8)


def mode4_rows(h: int, hu: int, wu: int, y0: int, y1: int) -> Tuple[Tuple[int, int], Tuple[int, int]]:
    """((ty0, ty1), (r0, r1)): the HR rows whose tap values mode 4 needs for output rows [y0,y1) (one more row each way,
    clipped to the image) and the LR rows those read (C ABI ``diinn_mode4_rows``)."""
    lib = _native.load()
    a, b, r0, r1 = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    _native.check(lib.diinn_mode4_rows(h, hu, wu, y0, y1, C.byref(a), C.byref(b), C.byref(r0), C.byref(r1)),
                  "diinn_mode4_rows")
    return (a.value, b.value), (r0.value, r1.value)


def lr_rows_for_band(h: int, hu: int, wu: int, y0: int, y1: int) -> Tuple[int, int]:
    """LR rows [r0,r1) whose cells HR rows [y0,y1) read (C ABI ``diinn_lr_rows_for_band``)."""
    lib = _native.load()
    r0, r1 = C.c_int(), C.c_int()
    _native.check(lib.diinn_lr_rows_for_band(h, hu, wu, y0, y1, C.byref(r0), C.byref(r1)),
                  "diinn_lr_rows_for_band")
    return r0.value, r1.value


# ---------------------------------------------------------------------------
# functional entry: features -> RGB on the current HIP stream
# ---------------------------------------------------------------------------
def _require_cuda(t: torch.Tensor, what: str) -> None:
    if not t.is_cuda:
        raise RuntimeError(
            f"diinn_amd: {what} must live on a ROCm GPU (got device {t.device}); the MI355X decode "
            f"path has no CPU implementation")


def require_2x2(hu: int, wu: int) -> None:
    """Mode 4's one size rule (nn.Conv2d's 'reflect' padding asks the same)."""
    if hu < 2 or wu < 2:
        raise ValueError(f"mode 4: the reflect-padded 3x3 head needs an output of at least 2 x 2, got {hu} x {wu}")


def _checked_feat(feat: torch.Tensor):
    """(``feat`` contiguous, (B, H, W)) of fp32 encoder features [B,64,H,W]."""
    if feat.dtype != torch.float32 or feat.dim() != 4 or feat.shape[1] != IN_CHANNELS:
        raise ValueError(f"feat must be fp32 [B,{IN_CHANNELS},H,W], got {feat.dtype} {tuple(feat.shape)}")
    b, _, h, w = feat.shape
    return feat.contiguous(), (b, h, w)


def _checked_out(out: Optional[torch.Tensor], shape, device, what: str = "out", dims: str = "[B,3,Hu,Wu]", owner: str = "feat"):
    """``out`` if it is a contiguous fp32 tensor of ``shape`` on ``device`` (a new one if None)."""
    if out is None:
        return torch.empty(shape, dtype=torch.float32, device=device)
    if out.shape != shape or out.dtype != torch.float32 or not out.is_contiguous() or out.device != device:
        raise ValueError(f"{what} must be a contiguous fp32 {dims} tensor on {owner}'s device")
    return out


def _checked_buffer(buf: Optional[torch.Tensor], need_bytes: int, device, what: str, fp32_required: bool, owner: str = "feat",
                    unit: str = "bytes"):
    """``buf`` if it is a contiguous buffer of at least ``need_bytes`` on ``device`` (a new fp32 one if None).  ``fp32_required``:
    ``pix`` and ``p_win`` must be fp32; ``workspace`` and ``taps`` are taken by their size alone."""
    if buf is None:
        return torch.empty(need_bytes // 4, dtype=torch.float32, device=device)
    if buf.numel() * buf.element_size() < need_bytes or (fp32_required and buf.dtype != torch.float32) or not buf.is_contiguous() \
            or buf.device != device:
        raise ValueError(f"{what} must be a contiguous {'fp32 ' if fp32_required else ''}buffer of >= "
                         f"{need_bytes if unit == 'bytes' else need_bytes // 4} {unit} on {owner}'s device")
    return buf


def _checked_head(head: Optional[torch.Tensor], hu: int, wu: int) -> None:
    if head is None:
        raise ValueError("mode 4 needs its 3x3 head image: head=pack_head3x3(state_dict) on feat's device")
    _require_cuda(head, "head image")
    require_2x2(hu, wu)


def _not_a_band(y0: int, y1: int, hu: int) -> ValueError:
    return ValueError(f"rows {(y0, y1)} are not a band of an image of {hu} rows")


def _launch(name: str, device, *args) -> None:
    """Enqueue the library's ``name`` on the current stream of ``device``: tensors go as their addresses, integers as they are."""
    with _native.launcher(device) as run:
        run(name, *args)


def decode_features(feat: torch.Tensor, packed: torch.Tensor, size: Sequence[int],
                    out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None,
                    rows: Optional[Tuple[int, int]] = None, sin_mode: int = _native.SIN_DEFAULT,
                    compute: str = "f32", mode: int = 3, head: Optional[torch.Tensor] = None,
                    taps: Optional[torch.Tensor] = None, initq: Optional[torch.Tensor] = None,
                    pix: Optional[torch.Tensor] = None, initq_x3: Optional[torch.Tensor] = None,
                    modes_x3: bool = False) -> torch.Tensor:
    """Decode encoder features ``feat`` [B,64,H,W] to RGB [B,3,Hu,Wu].

    ``rows=(y0,y1)`` computes only that HR row band (tile sharding across GPUs);
    the rest of ``out`` is left untouched.  ``workspace`` is the P image
    [B,H,W,1024] fp32 (allocated if None).  ``compute`` = "f32" (reference precision), "bf16" /
    "bf16_full" (bf16 operands in layers 1..3 / also in the hoisted conv, fp32 accumulate; ~2e-3 relative) or
    "bf16x3" (split bf16: hi + lo bf16 operands, three bf16 MFMA products per term; held to f32's 1e-4 bound).  ``mode`` 3 (default) is the
    reference's final model; modes 1 and 2 (packed with ``pack_state_dict(..., mode=...)``) run fp32
    only.  Mode 4 (fp32 only) takes the body image as ``packed`` (``pack_state_dict(..., mode=4)``) and the 3x3 head
    image as ``head`` (``pack_head3x3``); ``taps`` is its second workspace, ``diinn_mode4_taps_bytes`` bytes for the
    rows decoded (allocated if None).  A row band of mode 4 is bit-identical to the same rows of a whole-image decode.
    ``initq`` (mode 3, fp32 only): the init_q image (``pack_initq``) of an ``init_q=True`` decoder, with ``packed`` the body image
    of ``initq_body_state_dict``; ``pix`` is its workspace, the pixel planes of the rows decoded (``diinn_initq_pix_bytes``,
    5,120 bytes per HR pixel; allocated if None; ``workspace`` is not used).  A row band is bit-identical to the same rows of a
    whole-image decode.  ``initq_x3`` (with ``initq``, mode 3, ``compute="bf16x3"`` only): the init_q split image (``pack_initq_x3``)
    opens the split-bf16 arithmetic for such a decoder (``initq_planes_x3_kernel``, ``decode_bf16x3_kernel<SIN | X3_INITQ>``; the
    same ``pix``); without it ``compute="bf16x3"`` refuses like the other bf16 arithmetics.
    ``modes_x3`` (default False; modes 1, 2 and 4 with ``compute="bf16x3"`` only): opens the split-bf16 arithmetic for those modes --
    the Q-only form of ``decode_bf16x3_kernel`` behind the fp32 P and per-cell chain (modes 1/2: C ABI ``diinn_decode_qonly_x3``), its
    tap form behind mode 3's ``"bf16x3"`` P and in front of the unchanged gather (mode 4: ``diinn_decode_mode4_x3``); the same images,
    ``rows``, ``out``, ``workspace`` and ``taps``, bands bit-identical to the same rows of a whole-image decode.
    Without it these modes refuse every ``compute`` but ``"f32"`` as before; with it ``"bf16"`` and ``"bf16_full"`` still refuse, and
    mode 3 and ``"f32"`` are what they are without it.
    Enqueues two kernels (three for modes 1/2: + the per-cell modulation chain; three for mode 4: + the 9-point
    gather) on the current stream; never synchronises."""
    lib = _native.load()
    if initq is not None:
        if mode != 3:
            raise NotImplementedError(f"init_q=True is covered for mode 3 only (got mode {mode})")
        if compute != "f32" and not (compute == "bf16x3" and initq_x3 is not None):
            raise ValueError("init_q=True runs in fp32 only")
        if compute == "f32" and initq_x3 is not None:
            raise ValueError("initq_x3 is the image of compute='bf16x3'")
    elif initq_x3 is not None:
        raise ValueError("initq_x3 goes with initq (an init_q=True decoder)")
    _require_cuda(feat, "feat")
    _require_cuda(packed, "packed weights")
    feat, (b, h, w) = _checked_feat(feat)
    hu, wu = size  # same unpack as the reference (diinn.py:96): raises unless len(size) == 2
    hu, wu = int(hu), int(wu)
    y0, y1 = (0, hu) if rows is None else (int(rows[0]), int(rows[1]))
    dev = feat.device
    out = _checked_out(out, (b, 3, hu, wu), dev)
    geometry = (b, h, w, hu, wu, y0, y1, int(sin_mode))
    if initq is not None:
        _require_cuda(initq, "init_q image")
        pneed = lib.diinn_initq_pix_bytes(b, wu, y1 - y0)
        if pneed == 0 or y0 < 0 or y1 > hu:
            raise _not_a_band(y0, y1, hu)
        pix = _checked_buffer(pix, pneed, dev, "pix", True)
        if initq_x3 is not None:
            _require_cuda(initq_x3, "init_q split image")
            _launch("diinn_decode_initq_x3", dev, feat, packed, initq, initq_x3, pix, out, *geometry)
        else:
            _launch("diinn_decode_initq", dev, feat, packed, initq, pix, out, *geometry)
        return out
    workspace = _checked_buffer(workspace, lib.diinn_workspace_bytes(b, h, w), dev, "workspace", False)
    if mode not in (1, 2, 3, 4):
        raise NotImplementedError(f"mode {mode}: the HIP path covers modes 1-4")
    x3 = bool(modes_x3) and mode != 3 and compute == "bf16x3"     # the opt-in: split bf16 for modes 1, 2 and 4
    if mode != 3 and compute != "f32" and not x3:
        raise ValueError("modes 1, 2 and 4 run in fp32 only")
    if mode == 4:
        _checked_head(head, hu, wu)
        tneed = lib.diinn_mode4_taps_bytes(b, hu, wu, y0, y1)
        if tneed == 0:
            raise _not_a_band(y0, y1, hu)
        taps = _checked_buffer(taps, tneed, dev, "taps", False)
        _launch("diinn_decode_mode4_x3" if x3 else "diinn_decode_mode4", dev, feat, packed, head, workspace, taps, out, *geometry)
    elif x3:
        _launch("diinn_decode_qonly_x3", dev, feat, packed, workspace, out, *geometry)
    else:
        _launch("diinn_decode_ex", dev, feat, packed, workspace, out, *geometry,
                _native.COMPUTE[compute] if mode == 3 else _native.COMPUTE_F32_QONLY)
    return out


def decode_features_initq(feat: torch.Tensor, packed: torch.Tensor, initq: torch.Tensor, size: Sequence[int], mode: int,
                          head: Optional[torch.Tensor] = None, taps: Optional[torch.Tensor] = None,
                          pix: Optional[torch.Tensor] = None, rows: Optional[Tuple[int, int]] = None,
                          out: Optional[torch.Tensor] = None, sin_mode: int = _native.SIN_DEFAULT,
                          planes_rows: Optional[int] = None, compute: str = "f32",
                          initq_x3: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``init_q=True`` with decoder modes 1, 2 and 4 (inference): encoder features ``feat`` [B,64,H,W] -> RGB [B,3,Hu,Wu].
    (Mode 3 is ``decode_features(..., initq=...)``, which keeps refusing these modes.)

    ``packed`` = ``pack_state_dict(initq_body_state_dict(sd), mode=mode)``, ``initq`` = ``pack_initq(sd)``, ``head`` (mode 4) =
    ``pack_head3x3(sd)``, all on feat's device.  ``rows=(y0,y1)`` computes only that HR row band, bit-identical to the same rows
    of a whole-image decode; the rest of ``out`` is left untouched.  ``pix``: the pixel planes, 5,120 bytes per HR pixel of the
    rows decoded -- for mode 4 of the tap rows [max(0, y0-1), min(Hu, y1+1)) (``diinn_initq_mode4_pix_bytes``), as is ``taps``
    (``diinn_mode4_taps_bytes``); both allocated if None.  ``planes_rows`` (mode 1): 512 (default; the planes kernel computes the 512
    GEMM rows mode 1 has, the chain takes its seeds from the biases) or 1280 (mode 2's form on the zero-widened image: the
    same bits).  ``compute`` = "f32" (default) or "bf16x3": the split-bf16 arithmetic (``initq_planes_x3_kernel``,
    ``pixel_chain_x3_kernel``, ``decode_bf16x3_kernel<SIN | X3_INITQ | X3_QONLY>`` or ``<.. | X3_TAPS>``), which needs
    ``initq_x3 = pack_initq_x3(sd)`` on feat's device; the same workspaces, bands bit-identical to the whole image.  Any other
    ``compute`` raises ``ValueError``.  Enqueues three kernels on the current stream; never synchronises."""
    lib = _native.load()
    if mode not in (1, 2, 4):
        raise NotImplementedError(f"decode_features_initq covers modes 1, 2 and 4 (mode 3: decode_features(..., initq=...)), got mode {mode}")
    if compute not in ("f32", "bf16x3"):
        raise ValueError(f"init_q=True with modes 1, 2 and 4 runs in 'f32' or 'bf16x3', got compute={compute!r}")
    if compute == "bf16x3" and initq_x3 is None:
        raise ValueError("compute='bf16x3' needs initq_x3, the init_q split image (pack_initq_x3)")
    if compute == "f32" and initq_x3 is not None:
        raise ValueError("initq_x3 is the image of compute='bf16x3'")
    if planes_rows not in ((None, 512, 1280) if mode == 1 else (None, 1280)):
        raise ValueError(f"planes_rows={planes_rows}: mode 1 takes 512 or 1280, modes 2 and 4 the 1280-row planes only")
    _require_cuda(feat, "feat")
    _require_cuda(packed, "packed weights")
    _require_cuda(initq, "init_q image")
    if initq_x3 is not None:
        _require_cuda(initq_x3, "init_q split image")
    feat, (b, h, w) = _checked_feat(feat)
    hu, wu = size
    hu, wu = int(hu), int(wu)
    y0, y1 = (0, hu) if rows is None else (int(rows[0]), int(rows[1]))
    dev = feat.device
    if mode == 4:
        _checked_head(head, hu, wu)
    out = _checked_out(out, (b, 3, hu, wu), dev)
    pneed = lib.diinn_initq_mode4_pix_bytes(b, hu, wu, y0, y1) if mode == 4 else \
        (lib.diinn_initq_pix_bytes(b, wu, y1 - y0) if 0 <= y0 < y1 <= hu else 0)
    if pneed == 0:
        raise _not_a_band(y0, y1, hu)
    pix = _checked_buffer(pix, pneed, dev, "pix", True)
    geometry = (b, h, w, hu, wu, y0, y1, int(sin_mode))
    if mode == 4:
        taps = _checked_buffer(taps, lib.diinn_mode4_taps_bytes(b, hu, wu, y0, y1), dev, "taps", False)
        if initq_x3 is not None:
            _launch("diinn_decode_initq_mode4_x3", dev, feat, packed, initq, initq_x3, head, pix, taps, out, *geometry)
        else:
            _launch("diinn_decode_initq_mode4", dev, feat, packed, initq, head, pix, taps, out, *geometry)
    else:
        entry = "diinn_decode_initq_mode1" if mode == 1 and planes_rows != 1280 else "diinn_decode_initq_mode2"
        if initq_x3 is not None:
            _launch(entry + "_x3", dev, feat, packed, initq, initq_x3, pix, out, *geometry)
        else:
            _launch(entry, dev, feat, packed, initq, pix, out, *geometry)
    return out


def window_rows(h: int, hu: int, wu: int, y0: int, y1: int) -> Tuple[Tuple[int, int], Tuple[int, int]]:
    """((feat_row0, feat_rows), (p_row0, p_rows)): the LR feature rows (cells + 3x3 halo) and the P rows that
    decoding HR rows [y0,y1) touches (C ABI ``diinn_window_rows``)."""
    lib = _native.load()
    a0, an, r0, rn = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    _native.check(lib.diinn_window_rows(h, hu, wu, y0, y1, C.byref(a0), C.byref(an), C.byref(r0), C.byref(rn)),
                  "diinn_window_rows")
    return (a0.value, an.value), (r0.value, rn.value)


def decode_window(feat_win: torch.Tensor, feat_row0: int, full_h: int, packed: torch.Tensor, size: Sequence[int],
                  rows: Tuple[int, int], p_win: Optional[torch.Tensor] = None, out_win: Optional[torch.Tensor] = None,
                  sin_mode: int = _native.SIN_DEFAULT, compute: str = "f32", mode: int = 3) -> torch.Tensor:
    """Decode HR rows ``rows=(y0,y1)`` from band-sized buffers (the multi-GPU row-band unit).

    ``feat_win`` [B,64,fr,W] holds LR rows [feat_row0, feat_row0+fr) of a map of height ``full_h`` and must
    cover the band's cells plus the 3x3 halo (``window_rows``).  ``p_win`` is a workspace of at least
    B*p_rows*W*1024 floats and ``out_win`` [B,3,y1-y0,Wu] the band of the output (both allocated if None).
    Bit-identical to the same rows of ``decode_features`` on the full map.  C ABI: ``diinn_decode_win``."""
    _require_cuda(feat_win, "feat_win")
    _require_cuda(packed, "packed weights")
    if feat_win.dtype != torch.float32 or feat_win.dim() != 4 or feat_win.shape[1] != IN_CHANNELS \
            or not feat_win.is_contiguous():
        raise ValueError(f"feat_win must be contiguous fp32 [B,{IN_CHANNELS},rows,W], got {feat_win.dtype} "
                         f"{tuple(feat_win.shape)}")
    hu, wu = size
    hu, wu = int(hu), int(wu)
    y0, y1 = int(rows[0]), int(rows[1])
    b, _, fr, w = feat_win.shape
    dev = feat_win.device
    (_, _), (r0, rn) = window_rows(int(full_h), hu, wu, y0, y1)
    p_win = _checked_buffer(p_win, b * rn * w * P_CHANNELS * 4, dev, "p_win", True, owner="feat_win", unit="floats")
    out_win = _checked_out(out_win, (b, 3, y1 - y0, wu), dev, "out_win", "[B,3,y1-y0,Wu]", "feat_win")
    _launch("diinn_decode_win", dev, feat_win, int(feat_row0), fr, packed, p_win, r0, rn, out_win, y0, y1 - y0,
            b, int(full_h), w, hu, wu, y0, y1, int(sin_mode), _window_compute(mode, compute))
    return out_win


def _window_compute(mode: int, compute: str) -> int:
    """The library's compute code of a window or tile decode: modes 1-3, modes 1 and 2 in fp32 only."""
    if mode not in (1, 2, 3):
        raise NotImplementedError(f"mode {mode}: windows and tiles cover modes 1-3 (mode 4's 3x3 head reads its "
                                  f"neighbours' rows and columns: decode it with decode_features(rows=...))")
    if mode != 3 and compute != "f32":
        raise ValueError("modes 1 and 2 run in fp32 only")
    return _native.COMPUTE[compute] if mode == 3 else _native.COMPUTE_F32_QONLY


def decode_tile(p_win: torch.Tensor, p_row0: int, shape: Sequence[int], packed: torch.Tensor, size: Sequence[int],
                rows: Tuple[int, int], cols: Tuple[int, int], out: torch.Tensor,
                sin_mode: int = _native.SIN_DEFAULT, compute: str = "f32", mode: int = 3) -> torch.Tensor:
    """Decode the HR tile rows x cols = [y0,y1) x [x0,x1) from a P window (``diinn_precompute_P_win``'s output: LR rows
    [p_row0, p_row0 + p_rows) of the [B,H,W,1024] image, ``shape`` = (B, H, W) of the full map) INTO ``out``, any fp32
    view of shape [B,3,y1-y0,x1-x0] with unit stride along x -- a tensor of its own or a window of a larger canvas;
    nothing else of the canvas is written.  Bit-identical to the same pixels of ``decode_features``.  The reference's
    analogue is ``batched_step``'s column strips (diinn.py:149-160).  C ABI: ``diinn_decode_tile_win``.

    ``mode`` 1 / 2 (fp32 only): ``p_win`` must already hold the per-cell modulation chain in slots 1..3 of the rows the
    tile reads (``diinn_cell_chain`` after ``diinn_precompute_P_win``)."""
    _require_cuda(p_win, "p_win")
    _require_cuda(packed, "packed weights")
    b, h, w = (int(v) for v in shape)
    hu, wu = int(size[0]), int(size[1])
    y0, y1 = int(rows[0]), int(rows[1])
    x0, x1 = int(cols[0]), int(cols[1])
    if out.dtype != torch.float32 or out.dim() != 4 or tuple(out.shape) != (b, 3, y1 - y0, x1 - x0) or out.device != p_win.device:
        raise ValueError(f"out must be an fp32 [B,3,{y1 - y0},{x1 - x0}] view on the P window's device, got {out.dtype} {tuple(out.shape)}")
    if out.stride(3) != 1 and x1 - x0 > 1:
        raise ValueError("out must have unit stride along x")
    if p_win.dtype != torch.float32 or not p_win.is_contiguous() or p_win.numel() % (b * w * P_CHANNELS):
        raise ValueError("p_win must be a contiguous fp32 buffer of B * rows * W * 1024 floats")
    _launch("diinn_decode_tile_win", p_win.device, p_win, int(p_row0), p_win.numel() // (b * w * P_CHANNELS), packed, out,
            out.stride(2), out.stride(1), out.stride(0), b, h, w, hu, wu, y0, y1, x0, x1, int(sin_mode), _window_compute(mode, compute))
    return out


# ---------------------------------------------------------------------------
# LIIF comparison decoder (reference liif.py)
# ---------------------------------------------------------------------------
def pack_liif_state_dict(sd, prefix: str = "imnet.") -> torch.Tensor:
    """``imnet`` of the reference LIIF (MLP 580 -> 256 x4 -> 3, liif.py:24, mlp.py) -> the DIINN packed image,
    with the slot mapping documented at ``diinn_liif_decode`` in include/diinn_hip.h: the 576 feature
    columns of layer 0 become the hoisted 3x3 conv, its 4 coordinate columns the Q0 table, layers 2/4/6
    the synthesis slots of the stacked per-pixel layers, layer 8 the RGB head."""
    w0 = _host_array(sd, prefix, "layers.0.weight", (HIDDEN, 580))
    mapped = {
        "K.0.0.weight": w0[:, :576], "K.0.0.bias": _host_array(sd, prefix, "layers.0.bias", (HIDDEN,)),
        "Q.0.0.weight": w0[:, 576:579], "Q.0.0.bias": w0[:, 579],
        "last_layer.weight": _host_array(sd, prefix, "layers.8.weight", (3, HIDDEN)),
        "last_layer.bias": _host_array(sd, prefix, "layers.8.bias", (3,)),
    }
    for i, layer in ((1, 2), (2, 4), (3, 6)):
        mapped[f"K.{i}.0.weight"] = np.zeros((HIDDEN, HIDDEN + 576), np.float32)
        mapped[f"K.{i}.0.bias"] = np.zeros((HIDDEN,), np.float32)
        mapped[f"Q.{i}.0.weight"] = _host_array(sd, prefix, f"layers.{layer}.weight", (HIDDEN, HIDDEN))
        mapped[f"Q.{i}.0.bias"] = _host_array(sd, prefix, f"layers.{layer}.bias", (HIDDEN,))
    return pack_state_dict(mapped, mode=3)


def liif_axis_tables(n_in: int, n_out: int, v: int) -> Tuple[np.ndarray, np.ndarray, float]:
    """Host tables (idx int32, rel fp32) and rel_cell of one axis for ensemble shift v (C ABI)."""
    lib = _native.load()
    idx = np.empty(n_out, np.int32)
    rel = np.empty(n_out, np.float32)
    cell = C.c_float()
    _native.check(lib.diinn_liif_make_axis_tables(n_in, n_out, v, idx.ctypes.data_as(_native._i32), _native.fptr(rel),
                                                  C.byref(cell)), "diinn_liif_make_axis_tables")
    return idx, rel, cell.value


def pack_liif_split(packed_host: torch.Tensor) -> torch.Tensor:
    """The split training image (``diinn_pack_split_train_host``) of a LIIF packed image on the host: pieces 1 / 3 of every
    k-step of its forward half are hi / lo of ``imnet.layers.{2,4,6}.weight`` -- what ``liif_x3_kernel`` streams."""
    from .split_training import pack_split_host
    return torch.from_numpy(pack_split_host(packed_host.detach().cpu().numpy()))


def _comparison_decode(name: str, workspace_bytes, feat: torch.Tensor, packed: torch.Tensor, size: Sequence[int],
                       out: Optional[torch.Tensor], workspace: Optional[torch.Tensor],
                       split: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The LIIF / MetaSR decode of every HR pixel: the library's ``name`` (diinn_liif_decode's signature; with ``split``, a
    second weight image behind ``packed``) with ``workspace_bytes(B, H, W)`` bytes of workspace; a ``workspace`` that is too
    small is replaced."""
    _require_cuda(feat, "feat")
    _require_cuda(packed, "packed weights")
    images = (packed,)
    if split is not None:
        _require_cuda(split, "split weights")
        if split.dtype != torch.float32 or not split.is_contiguous() or split.numel() != _native.load().diinn_split_train_floats() \
                or split.device != packed.device:
            raise ValueError("split must be the contiguous fp32 split training image of packed (pack_liif_split) on its device")
        images = (packed, split)
    feat, (b, h, w) = _checked_feat(feat)
    hu, wu = size
    hu, wu = int(hu), int(wu)
    out = _checked_out(out, (b, 3, hu, wu), feat.device)
    need = workspace_bytes(b, h, w)
    if workspace is None or workspace.numel() * 4 < need or workspace.device != feat.device:
        workspace = torch.empty(need // 4, dtype=torch.float32, device=feat.device)
    _launch(name, feat.device, feat, *images, workspace, out, b, h, w, hu, wu)
    return out


def liif_decode_features(feat: torch.Tensor, packed: torch.Tensor, size: Sequence[int],
                         out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None,
                         split: Optional[torch.Tensor] = None) -> torch.Tensor:
    """LIIF query of every HR pixel: encoder features [B,64,H,W] -> RGB [B,3,Hu,Wu] (liif.py:59-127,148-155).

    ``split`` (opt-in, not in the reference): the split training image of ``packed`` (``pack_liif_split``) on its device.  The
    three hidden 256 x 256 layers of every ensemble member then run in split-bf16 arithmetic (``diinn_liif_decode_x3``,
    ``liif_x3_kernel``; sheet: ``liif_x3_forward_reference``) -- within the fp32 contract, 1e-4 x max(1, max|ref|), but not
    ``liif_kernel``'s bits."""
    if split is None:
        return _comparison_decode("diinn_liif_decode", _native.load().diinn_workspace_bytes, feat, packed, size, out, workspace)
    return _comparison_decode("diinn_liif_decode_x3", _native.load().diinn_workspace_bytes, feat, packed, size, out, workspace,
                              split=split)


# ---------------------------------------------------------------------------
# MetaSR comparison decoder (reference metasr.py)
# ---------------------------------------------------------------------------
def pack_metasr_state_dict(sd, prefix: str = "imnet.") -> torch.Tensor:
    """``imnet`` of the reference MetaSR (Linear(3,256), ReLU, Linear(256,1728); metasr.py:27-35) -> its packed
    image (C ABI ``diinn_metasr_pack_weights``)."""
    lib = _native.load()

    w1, b1 = _host_array(sd, prefix, "layers.0.weight", (HIDDEN, 3)), _host_array(sd, prefix, "layers.0.bias", (HIDDEN,))
    w2, b2 = _host_array(sd, prefix, "layers.2.weight", (1728, HIDDEN)), _host_array(sd, prefix, "layers.2.bias", (1728,))
    packed = np.empty(lib.diinn_metasr_packed_floats(), dtype=np.float32)
    _native.check(lib.diinn_metasr_pack_weights(_native.fptr(w1), _native.fptr(b1), _native.fptr(w2), _native.fptr(b2),
                                                _native.fptr(packed)), "diinn_metasr_pack_weights")
    return torch.from_numpy(packed)


def metasr_axis_tables(n_in: int, n_out: int) -> Tuple[np.ndarray, np.ndarray, float]:
    lib = _native.load()
    idx = np.empty(n_out, np.int32)
    rel = np.empty(n_out, np.float32)
    r_rev = C.c_float()
    _native.check(lib.diinn_metasr_make_axis_tables(n_in, n_out, idx.ctypes.data_as(_native._i32), _native.fptr(rel),
                                                    C.byref(r_rev)), "diinn_metasr_make_axis_tables")
    return idx, rel, r_rev.value


def metasr_decode_features(feat: torch.Tensor, packed: torch.Tensor, size: Sequence[int],
                           out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """MetaSR query of every HR pixel: encoder features [B,64,H,W] -> RGB [B,3,Hu,Wu] (metasr.py:70-104,125-135)."""
    return _comparison_decode("diinn_metasr_decode", _native.load().diinn_metasr_workspace_bytes, feat, packed, size, out, workspace)


def metasr_decode_hoisted(feat: torch.Tensor, packed: torch.Tensor, image: torch.Tensor, size: Sequence[int],
                          out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None,
                          rows: Optional[Tuple[int, int]] = None) -> torch.Tensor:
    """The same MetaSR query in the hoisted form (``metasr_training``'s docstring; opt-in, not the reference's bits): the 3x3 conv
    [M; B0] of the whole map per LR cell (``diinn_precompute_P_wpu`` on ``image``, the DIINN-shaped training image of
    ``metasr_training.images_on_device``, into ``workspace``: ``diinn_workspace_bytes(B,H,W)`` bytes, replaced if too small),
    then ``diinn_metasr_decode_hoisted`` on ``packed`` (the MetaSR image of the same call; its W1 / b1 rows).  ``rows=(y0,y1)``
    writes only that HR row window of a full-size ``out``.  Measured faster than the direct decode at every scale tried, x0.33 to x4
    (17x at 256 x 256 x4, 1.1x below x1: DESIGN.md §3.8, profiles/metasr_hoisted_times.txt)."""
    _require_cuda(feat, "feat")
    _require_cuda(packed, "packed weights")
    _require_cuda(image, "training image")
    feat, (b, h, w) = _checked_feat(feat)
    hu, wu = int(size[0]), int(size[1])
    y0, y1 = (0, hu) if rows is None else (int(rows[0]), int(rows[1]))
    if not 0 <= y0 <= y1 <= hu:
        raise ValueError(f"rows must satisfy 0 <= y0 <= y1 <= {hu}, got ({y0}, {y1})")
    out = _checked_out(out, (b, 3, hu, wu), feat.device)
    need = _native.load().diinn_workspace_bytes(b, h, w)
    if workspace is None or workspace.numel() * 4 < need or workspace.device != feat.device:
        workspace = torch.empty(need // 4, dtype=torch.float32, device=feat.device)
    with _native.launcher(feat.device) as run:
        run("diinn_precompute_P_wpu", feat, image, workspace, b, h, w, 0, h)
        run("diinn_metasr_decode_hoisted", workspace, packed, out, b, h, w, hu, wu, y0, y1)
    return out


# ---------------------------------------------------------------------------
# nn.Module mirror of the reference class
# ---------------------------------------------------------------------------
class ImplicitDecoder(nn.Module):
    """Drop-in for the reference ``ImplicitDecoder`` (diinn.py:39-173).

    Every mode registers the reference's parameters (so any reference checkpoint
    loads); the MI355X kernels implement the paper's final variant, ``mode=3,
    init_q=False`` (README.md:111-112 of the reference), the ablation modes 1 and 2, whose
    modulation branch depends on the LR cell only, and mode 4, mode 3 with a 3x3 reflect-padded
    head (fp32; inference, and training with ``hip_autograd_mode4``).  ``init_q=True`` (the per-pixel sine embedding ``first_layer``, diinn.py:48-51,113-115) runs
    for mode 3, inference, fp32; with modes 1, 2, 4 (unless ``hip_initq_modes`` is set, below) or under autograd ``forward`` raises
    ``NotImplementedError``.

    Nine opt-ins, each a plain attribute and a constructor keyword, default False.  Each opens exactly one more combination of
    (mode, ``init_q``, ``compute``, inference or autograd) and changes nothing for any other; "autograd" is ``forward(x, size,
    None)`` with grad enabled and something requiring it (``bsize`` given, or ``no_grad``, is the inference path, like the
    reference's ``batched_step``).  ``_route`` is the rule -- one table, every supported combination, the flag that opens it and
    the refusal everything else gets -- and ``tests/test_decoder_routes.py`` pins it for every setting of the first seven (the eighth:
    ``tests/test_initq_split_training.py``; the ninth: ``tests/test_decoder_initq_modes_x3.py``).

    ==================================  ==========================================  ===========================  =============================
    flag                                opens                                       needs beside it              what keeps refusing with it
    ==================================  ==========================================  ===========================  =============================
    ``hip_autograd``                    autograd, ``init_q``, mode 3, fp32          --                           init_q modes 1/2/4, mode 4,
                                        (``initq_training``)                                                     every bf16 arithmetic
    ``hip_autograd_mode4``              autograd, mode 4, ``init_q=False``, fp32    output >= 2 x 2              mode 4 with ``init_q`` or a
                                        (``mode4_training``)                                                     bf16 arithmetic
    ``hip_initq_modes``                 inference, ``init_q``, modes 1/2/4, fp32    --                           autograd, bf16 arithmetics,
                                        (``decode_features_initq``)                                 ``graphs=True``, sharded
    ``hip_initq_split_bf16``            inference, ``init_q``, mode 3, "bf16x3"     ``compute="bf16x3"``         "bf16", "bf16_full", autograd,
                                                                                                 init_q modes 1/2/4, graphs,
                                                                                                                 sharded
    ``hip_autograd_initq_modes``        autograd, ``init_q``, modes 1/2/4, fp32     ``hip_initq_modes``          bf16 arithmetics, graphs,
                                        (``initq_modes_training``)     (alone it does nothing)      sharded
    ``hip_autograd_split_bf16``         autograd, mode 3, ``init_q=False``,         ``compute="bf16x3"``         modes 1/2/4 and ``init_q``
                                        "bf16x3" both ways (``split_training``;                                  in "bf16x3" under autograd,
                                        DESIGN.md 3.7f)                                                          "bf16", "bf16_full", graphs,
                                                                                                                 sharded
    ``hip_modes_split_bf16``            inference, modes 1/2/4, ``init_q=False``,   ``compute="bf16x3"``         autograd in "bf16x3", init_q
                                        "bf16x3" (``decode_features(modes_x3=       (``graphs=True`` replays     modes 1/2/4 in any bf16,
                                        True)``)                    it)                          "bf16", "bf16_full", sharded
    ``hip_autograd_initq_split_bf16``   autograd, ``init_q``, mode 3, "bf16x3"      ``compute="bf16x3"`` and     init_q modes 1/2/4 in any
                                        both ways (``initq_split_training``;        ``hip_initq_split_bf16``     bf16, "bf16", "bf16_full",
                                        DESIGN.md 3.7g)                             (alone it does nothing)      graphs, sharded
    ``hip_initq_modes_split_bf16``      inference, ``init_q``, modes 1/2/4,         ``compute="bf16x3"`` and     autograd in "bf16x3", "bf16",
                                        "bf16x3" (``decode_features_initq(          ``hip_initq_modes``          "bf16_full", graphs, sharded
                                        compute="bf16x3")``)        (alone it does nothing)
    ==================================  ==========================================  ===========================  =============================

    ``compute="f32"`` gives the fp32 bits whatever is set.  ``DIINN.set_split_bf16()`` sets none of the five split flags: a user who
    wants the split arithmetic on such a model sets both."""

    hip_autograd = False
    hip_autograd_mode4 = False
    hip_initq_modes = False
    hip_initq_split_bf16 = False
    hip_autograd_initq_modes = False
    hip_autograd_split_bf16 = False
    hip_modes_split_bf16 = False
    hip_autograd_initq_split_bf16 = False
    hip_initq_modes_split_bf16 = False

    def __init__(self, in_channels: int = 64, hidden_dims=(256, 256, 256, 256), mode: int = 1,
                 init_q: bool = False, sin_mode: int = _native.SIN_DEFAULT, compute: str = "f32", hip_autograd: bool = False,
                 hip_autograd_mode4: bool = False, hip_initq_modes: bool = False, hip_initq_split_bf16: bool = False,
                 hip_autograd_initq_modes: bool = False, hip_autograd_split_bf16: bool = False,
                 hip_modes_split_bf16: bool = False, hip_autograd_initq_split_bf16: bool = False,
                 hip_initq_modes_split_bf16: bool = False):
        super().__init__()
        self.mode = mode
        self.init_q = init_q
        self.hip_autograd = bool(hip_autograd)
        self.hip_autograd_mode4 = bool(hip_autograd_mode4)
        self.hip_initq_modes = bool(hip_initq_modes)
        self.hip_initq_split_bf16 = bool(hip_initq_split_bf16)
        self.hip_autograd_initq_modes = bool(hip_autograd_initq_modes)
        self.hip_autograd_split_bf16 = bool(hip_autograd_split_bf16)
        self.hip_modes_split_bf16 = bool(hip_modes_split_bf16)
        self.hip_autograd_initq_split_bf16 = bool(hip_autograd_initq_split_bf16)
        self.hip_initq_modes_split_bf16 = bool(hip_initq_modes_split_bf16)
        self.in_channels = in_channels
        self.hidden_dims = list(hidden_dims)
        self.sin_mode = sin_mode
        self.compute = compute            # "f32" (default, reference precision), "bf16", "bf16_full" or "bf16x3"
        unfolded = in_channels * 9
        if init_q:
            self.first_layer = nn.Sequential(nn.Conv2d(3, unfolded, 1), SineAct())
        self.K = nn.ModuleList()
        self.Q = nn.ModuleList()
        k_in, q_in = unfolded, (unfolded if init_q else 3)
        for width in self.hidden_dims:
            self.K.append(nn.Sequential(nn.Conv2d(k_in, width, 1), nn.ReLU()))
            self.Q.append(nn.Sequential(nn.Conv2d(q_in, width, 1), SineAct()))
            # mode 1 chains k -> K[i]; modes 2-4 feed [k or q ; unfolded features] (diinn.py:53-88)
            k_in = width if mode == 1 else width + unfolded
            q_in = width
        if mode == 4:
            self.last_layer = nn.Conv2d(self.hidden_dims[-1], 3, 3, padding=1, padding_mode="reflect")
        else:
            self.last_layer = nn.Conv2d(self.hidden_dims[-1], 3, 1)
        self._packed: Optional[torch.Tensor] = None
        self._packed_key = None
        # P workspaces, one per (device, stream) that called forward: two streams decoding through one module concurrently
        # must not share the hoisted conv's image (at most _MAX_WORKSPACES kept, oldest dropped)
        self._workspaces: "Dict[tuple, torch.Tensor]" = {}
        # mode 4: the head image (cached with the body image) and the tap workspaces, kept like the P workspaces
        self._packed_head: Optional[torch.Tensor] = None
        self._tap_workspaces: "Dict[tuple, torch.Tensor]" = {}
        # init_q (mode 3): the first-layer / Q.0 image (cached with the body image) and the pixel-plane workspaces
        self._packed_initq: Optional[torch.Tensor] = None
        self._packed_initq_x3: Optional[torch.Tensor] = None     # the split image (bf16x3), packed and cached with them
        self._pix_workspaces: "Dict[tuple, torch.Tensor]" = {}

    _MAX_WORKSPACES = 4
    # init_q decodes in chunks of HR rows whose pixel planes (5,120 bytes per pixel) stay within this many bytes: a memory cap
    # (a 1024 x 1024 output would need 5 GiB at once), not a tuned number
    INITQ_CHUNK_BYTES = 256 * 1024 * 1024
    # mode 4 decodes at most this many HR rows per call, which caps the tap buffer at B x 256 x Wu x 112 bytes.  254, not 256: a
    # middle chunk needs the tap values of one more row each way, and 256 tap rows are a whole number of decode_kernel's 8-row
    # blocks (258 rows start a 33rd block row: at 1024 x 1024 a ninth round of workgroups per chunk, 7.40 against 6.47 ms measured)
    MODE4_CHUNK_ROWS = 254

    # -- packed-weight cache ---------------------------------------------------
    def _weights_key(self, device):
        return (str(device),) + tuple((p.data_ptr(), p._version) for p in self.parameters())

    def packed_weights(self, device) -> torch.Tensor:
        key = self._weights_key(device)
        if self._packed is None or self._packed_key != key:
            sd = self.state_dict()
            self._packed = pack_state_dict(initq_body_state_dict(sd) if self.init_q else sd, mode=self.mode).to(device)
            self._packed_head = pack_head3x3(sd).to(device) if self.mode == 4 else None
            self._packed_initq = pack_initq(sd).to(device) if self.init_q else None
            self._packed_initq_x3 = pack_initq_x3(sd).to(device) if self.init_q else None
            self._packed_key = key
        return self._packed

    def packed_head(self, device) -> torch.Tensor:
        """Mode 4: the 3x3 head image on ``device`` (packed and cached together with the body image)."""
        if self.mode != 4:
            raise ValueError("only mode 4 has a 3x3 head image")
        self.packed_weights(device)
        return self._packed_head

    def packed_initq(self, device) -> torch.Tensor:
        """``init_q=True``: the first-layer / Q.0 image on ``device`` (packed and cached together with the body image)."""
        if not self.init_q:
            raise ValueError("only init_q=True has an init_q image")
        self.packed_weights(device)
        return self._packed_initq

    def packed_initq_x3(self, device) -> torch.Tensor:
        """``init_q=True``: the init_q split image on ``device`` (packed and cached together with the body image)."""
        if not self.init_q:
            raise ValueError("only init_q=True has an init_q split image")
        self.packed_weights(device)
        return self._packed_initq_x3

    # -- which combination runs where ---------------------------------------------
    _NO_AUTOGRAD = (NotImplementedError,
                    "diinn_amd: autograd through the HIP decode path covers modes 1-3 in fp32 with init_q=False (mode 3 is the "
                    "reference's final model, modes 1/2 its ablations); call mode 4, init_q=True or the bf16 path under "
                    "torch.no_grad() (mode 4 in fp32 with init_q=False trains once ImplicitDecoder.hip_autograd_mode4 is set)")
    _INFERENCE_ONLY = (NotImplementedError,
                       "diinn_amd: init_q=True with mode {mode} (ImplicitDecoder.hip_initq_modes) is inference only: autograd "
                       "through it is not covered, and hip_autograd / hip_autograd_mode4 do not open it; call it under "
                       "torch.no_grad() or with bsize given")
    _INITQ_FP32_ONLY = (ValueError, "init_q=True runs in fp32 only")
    # Rows of (route or refusal, modes, init_q, compute, flags that must be set); None = any; the first row that matches decides.
    # _check_supported has already refused init_q with modes 1/2/4 unless hip_initq_modes is set.
    _INFERENCE_ROUTES = (
        ("plain",           (1, 2, 3),    False, None,        ()),    # decode_features refuses modes 1/2 in a bf16 arithmetic
        #                                                               (in "bf16x3": unless hip_modes_split_bf16 is set)
        ("mode4",           (4,),         False, ("f32",),    ()),
        ("mode4",           (4,),         False, ("bf16x3",), ("hip_modes_split_bf16",)),
        ("mode4_fp32_only", (4,),         False, None,        ()),    # refused behind the device check: "mode 4 runs in fp32 only"
        ("initq",           (3,),         True,  ("f32",),    ()),
        ("initq",           (3,),         True,  ("bf16x3",), ("hip_initq_split_bf16",)),
        ("initq_modes",     (1, 2, 4),    True,  ("f32",),    ("hip_initq_modes",)),
        ("initq_modes",     (1, 2, 4),    True,  ("bf16x3",), ("hip_initq_modes", "hip_initq_modes_split_bf16")),
        (_INITQ_FP32_ONLY,  (1, 2, 3, 4), True,  None,        ()),
    )
    _AUTOGRAD_ROUTES = (
        ("grad",             (1, 2, 3),    False, ("f32",),    ()),
        ("grad_split",       (3,),         False, ("bf16x3",), ("hip_autograd_split_bf16",)),
        ("grad_mode4",       (4,),         False, ("f32",),    ("hip_autograd_mode4",)),
        ("grad_initq",       (3,),         True,  ("f32",),    ("hip_autograd",)),
        ("grad_initq_modes", (1, 2, 4),    True,  ("f32",),    ("hip_initq_modes", "hip_autograd_initq_modes")),
        ("grad_initq_split", (3,),         True,  ("bf16x3",), ("hip_initq_split_bf16", "hip_autograd_initq_split_bf16")),
        (_INFERENCE_ONLY,    (1, 2, 4),    True,  None,        ()),
        (_NO_AUTOGRAD,       (1, 2, 3, 4), None,  None,        ()),
    )
    # the module whose decode_with_grad runs an autograd route
    _GRAD_MODULES = {"grad": "training", "grad_split": "split_training", "grad_mode4": "mode4_training",
                     "grad_initq": "initq_training", "grad_initq_modes": "initq_modes_training",
                     "grad_initq_split": "initq_split_training"}

    def _route(self, wants_grad: bool) -> str:
        """The path of this (mode, init_q, compute) with the flags as they are set, under autograd or not: a route name, or the
        refusal raised.  Decides and nothing else; looks at no tensor."""
        init_q = bool(self.init_q)
        for route, modes, q, computes, flags in (self._AUTOGRAD_ROUTES if wants_grad else self._INFERENCE_ROUTES):
            if self.mode in modes and (q is None or q == init_q) and (computes is None or self.compute in computes) \
                    and all(getattr(self, flag) for flag in flags):
                if isinstance(route, str):
                    return route
                raise route[0](route[1].format(mode=self.mode))
        raise AssertionError("every supported (mode, init_q) has a closing row")

    def _check_supported(self):
        if self.mode not in (1, 2, 3, 4) or (self.init_q and self.mode != 3 and not self.hip_initq_modes):
            raise NotImplementedError(
                f"diinn_amd HIP decode path implements modes 1-4 with init_q=False (mode 3 is the reference's "
                f"final model) and init_q=True for mode 3, which is covered; got mode={self.mode}, init_q={self.init_q}")
        if self.in_channels != IN_CHANNELS or self.hidden_dims != [HIDDEN] * 4:
            raise NotImplementedError("diinn_amd HIP decode path is built for in_channels=64, hidden_dims=[256]*4")

    def forward(self, x: torch.Tensor, size, bsize: Optional[int] = None) -> torch.Tensor:
        """x [B,64,H,W] fp32 encoder features, size=(H_up, W_up) -> [B,3,H_up,W_up].

        ``bsize`` is the reference's column-strip size (diinn.py:149-160), a
        memory knob there.  The fused kernels keep every per-pixel intermediate
        in registers, so it is accepted and ignored (results are identical for
        any value; the reference's hang for bsize < H_up cannot occur).

        Mode 4: the reference's ``batched_step`` applies the head's reflect padding at every column-strip edge, so
        the reference's own result depends on ``bsize`` there.  This path reproduces ``bsize=None``, the whole-image
        convolution, for any ``bsize``.  fp32; the image is decoded in chunks
        of at most ``MODE4_CHUNK_ROWS`` HR rows, which bounds the tap workspace and changes no bit of the result.
        Under autograd with ``bsize=None`` it raises unless ``hip_autograd_mode4`` is set (then:
        ``mode4_training.DecodeMode4Function``, the whole image at once).

        ``init_q=True`` (mode 3, fp32, inference only): the per-pixel planes the two kernels hand over take 5,120 bytes per
        HR pixel, so the image is decoded in chunks of ``initq_chunk_rows(B, W_up, INITQ_CHUNK_BYTES)`` HR rows; chunking
        changes no bit of the result either.  ``bsize=30000`` and ``bsize=None`` give the same bits, as in the reference.
        Under autograd with ``bsize=None`` it raises unless ``hip_autograd`` is set (then: ``initq_training.DecodeInitqFunction``,
        the whole image at once).

        ``init_q=True`` with modes 1, 2, 4 (``hip_initq_modes`` set; fp32, or ``"bf16x3"`` with ``hip_initq_modes_split_bf16`` set as
        well; inference only): the same chunks of HR rows in either arithmetic; mode 4
        computes the planes and the taps of a chunk's rows plus one row each way, clipped to the image, and it is those
        ``initq_chunk_rows`` rows that stay within the cap (a chunk is two output rows shorter).  Chunks change no bit,
        ``bsize`` is ignored, and mode 4 reproduces ``bsize=None`` as it does without ``init_q``.  Under autograd with ``bsize=None``
        it raises unless ``hip_autograd_initq_modes`` is set as well (then: ``initq_modes_training.DecodeInitqModesFunction``, the
        whole image at once)."""
        self._check_supported()
        # reference: bsize=None runs step() under autograd (training, sr_module.py:128).  What this path cannot
        # differentiate is refused before anything looks at the tensor's device: the answer depends on no tensor data
        wants_grad = bsize is None and torch.is_grad_enabled() and (
            x.requires_grad or any(p.requires_grad for p in self.parameters()))
        route = self._route(wants_grad)
        if wants_grad:
            if self.mode == 4:
                require_2x2(int(size[0]), int(size[1]))
            _require_cuda(x, "x")
            return importlib.import_module("." + self._GRAD_MODULES[route], __package__).decode_with_grad(self, x, size)
        _require_cuda(x, "x")
        b, _, h, w = x.shape
        x3 = self.compute == "bf16x3"                 # on a chunked route: the opt-in that opened it is set
        if route == "plain":
            workspace = self._workspace(self._workspaces, b * h * w * P_CHANNELS, x.device)
            with torch.no_grad():
                return decode_features(x, self.packed_weights(x.device), size, workspace=workspace, sin_mode=self.sin_mode,
                                       compute=self.compute, mode=self.mode,
                                       modes_x3=bool(self.hip_modes_split_bf16 and self.mode != 3 and x3))
        if route == "mode4":
            workspace = self._workspace(self._workspaces, b * h * w * P_CHANNELS, x.device)
            return self._decode_chunks(x, size, self.MODE4_CHUNK_ROWS, 0, lambda packed, out, rows, pix, taps: decode_features(
                x, packed, out.shape[2:], out=out, workspace=workspace, rows=rows, sin_mode=self.sin_mode, mode=4,
                head=self._packed_head, taps=taps, compute="bf16x3" if x3 else "f32", modes_x3=x3))
        if route == "mode4_fp32_only":
            raise ValueError("mode 4 runs in fp32 only")
        chunk = initq_chunk_rows(b, int(size[1]), self.INITQ_CHUNK_BYTES)
        if route == "initq":
            return self._decode_chunks(x, size, chunk, 0, lambda packed, out, rows, pix, taps: decode_features(
                x, packed, out.shape[2:], out=out, rows=rows, sin_mode=self.sin_mode, initq=self._packed_initq, pix=pix,
                compute="bf16x3" if x3 else "f32", initq_x3=self._packed_initq_x3 if x3 else None))
        # route == "initq_modes".  Mode 4 computes the planes and the taps of one more row each way (clipped to the image): THOSE
        # rows follow the chunk rule -- within the cap and a whole number of the kernels' 8-row blocks, as MODE4_CHUNK_ROWS = 254
        # does without init_q -- so a chunk is two output rows shorter (16 + 2 tap rows would start a third block row of both
        # kernels: B = 16 of 48 x 48 x4 measured 22.8 ms that way against the eager sequence's 21.4)
        halo = 2 if self.mode == 4 else 0
        # (fp32: the call as it always was; the split arithmetic adds its two keywords)
        return self._decode_chunks(x, size, chunk - halo, halo, lambda packed, out, rows, pix, taps: decode_features_initq(
            x, packed, self._packed_initq, out.shape[2:], self.mode, head=self._packed_head, taps=taps, pix=pix, rows=rows, out=out,
            sin_mode=self.sin_mode, **({"compute": "bf16x3", "initq_x3": self._packed_initq_x3} if x3 else {})))

    def _workspace(self, cache, numel: int, device) -> torch.Tensor:
        """An fp32 buffer of at least ``numel`` from ``cache``, one per (device, stream) that called forward."""
        # hipGraph capture (modules._GraphReplay): the captured kernels keep the workspace pointer for the
        # graph's lifetime, so it must come from the graph's private pool -- the cached workspace is
        # replaced (and its block recycled) as soon as a larger input arrives
        if torch.cuda.is_current_stream_capturing():
            return torch.empty(numel, dtype=torch.float32, device=device)
        key = (str(device), torch.cuda.current_stream(device).cuda_stream)
        ws = cache.get(key)
        if ws is None or ws.numel() < numel:
            cache.pop(key, None)
            while len(cache) >= self._MAX_WORKSPACES:
                cache.pop(next(iter(cache)))
            ws = cache[key] = torch.empty(numel, dtype=torch.float32, device=device)
        return ws

    def _decode_chunks(self, x: torch.Tensor, size, chunk: int, halo: int, decode) -> torch.Tensor:
        """The image in bands of ``chunk`` HR rows: ``decode(packed, out, rows, pix, taps)`` per band into one ``out``.  ``pix``
        (``init_q``) holds the planes of a band plus ``halo`` rows, ``taps`` (mode 4) those of the largest band: rows
        [0, chunk + 1) reach one tap row each way unless the image ends first."""
        b = x.shape[0]
        hu, wu = size
        hu, wu = int(hu), int(wu)
        pix = taps = None
        if self.mode == 4:
            require_2x2(hu, wu)
            taps = self._workspace(self._tap_workspaces, _native.load().diinn_mode4_taps_bytes(b, hu, wu, 1, min(hu, chunk + 1)) // 4,
                                   x.device)
        if self.init_q:
            pix = self._workspace(self._pix_workspaces, b * min(chunk + halo, hu) * wu * (P_CHANNELS + HIDDEN), x.device)
        with torch.no_grad():
            packed = self.packed_weights(x.device)
            out = torch.empty((b, 3, hu, wu), dtype=torch.float32, device=x.device)
            for y0 in range(0, hu, chunk):
                decode(packed, out, (y0, min(hu, y0 + chunk)), pix, taps)
        return out
