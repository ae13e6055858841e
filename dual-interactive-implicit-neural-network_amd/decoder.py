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
import math
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn as nn

from . import _native

IN_CHANNELS = 64
HIDDEN = 256
P_CHANNELS = 1024


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


INV_2PI_F32 = float(np.float32(0.15915494309189533577))     # fp32(1 / (2 pi)): the factor the host packers multiply by


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


def _split_bf16(v: torch.Tensor):
    """hi = bf16(v), lo = bf16(v - hi) (round to nearest even), both back in v's dtype."""
    hi = v.to(torch.bfloat16).to(v.dtype)
    return hi, (v - hi).to(torch.bfloat16).to(v.dtype)


def _mm_split(w: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    """The split-bf16 product of DESIGN.md 3.5: (w_lo . x_hi + w_hi . x_lo) + w_hi . x_hi, accumulated in the operands' dtype."""
    wh, wl = _split_bf16(w)
    xh, xl = _split_bf16(x)
    return (wl @ xh + wh @ xl) + wh @ xh


def _sin_rev(a: torch.Tensor) -> torch.Tensor:
    """sin of an argument in revolutions, taken in float64 and rounded to the argument's dtype."""
    return torch.sin(a.double() * (2.0 * math.pi)).to(a.dtype)


def initq_planes_reference(sd, feat, size, arith: str = "split", prefix: str = "") -> torch.Tensor:
    """The pixel planes of the split-bf16 ``init_q`` path, [B, Hu*Wu, 1280] (channels 1024.. in REVOLUTIONS), as
    ``initq_planes_x3_kernel`` forms them: everything that feeds a sine divided by fp32(1/(2 pi)) in fp32, ``E`` by the kernel's
    fp32 fma sequence (ratio, rel_w, rel_h) with the sine taken in float64, ``x' = E * X`` in fp32.  ``arith`` = "split": both GEMMs
    as ``_mm_split`` in fp32 (torch matmuls, not the MFMA's summation order); "f64": the float64 products of the same fp32
    operands, the yardstick of the planes test."""
    if arith not in ("split", "f64"):
        raise ValueError(f"arith must be 'split' or 'f64', got {arith!r}")
    f32 = torch.float32
    dev = feat.device

    def get(name, shape):
        t = sd[prefix + name]
        t = t.detach() if isinstance(t, torch.Tensor) else torch.from_numpy(np.asarray(t))
        return t.to(device=dev, dtype=f32).reshape(shape)

    inv = torch.tensor(INV_2PI_F32, dtype=f32, device=dev)
    hu, wu = int(size[0]), int(size[1])
    x = feat.to(f32)
    b, c, h, w = x.shape
    small = bool(_native.load().diinn_uses_small_output_kernel(hu, wu))
    iy, rel_h = axis_tables(h, hu, small)
    ix, rel_w = axis_tables(w, wu, small)
    iy_t, ix_t = torch.from_numpy(iy.astype(np.int64)).to(dev), torch.from_numpy(ix.astype(np.int64)).to(dev)
    n = hu * wu
    relh = torch.from_numpy(rel_h).to(dev, f32)[:, None].expand(hu, wu).reshape(1, n)
    relw = torch.from_numpy(rel_w).to(dev, f32)[None, :].expand(hu, wu).reshape(1, n)
    ratio = torch.tensor(np.float32((h * w) / (hu * wu)), dtype=f32, device=dev)
    fw, fb = get("first_layer.0.weight", (576, 3)) * inv, get("first_layer.0.bias", (576, 1)) * inv

    def fma(a_, b_, c_):                                      # one rounding: the fp32 product is exact in float64
        return (a_.double() * b_.double() + c_.double()).to(f32)

    a = fma(fw[:, 2:3], ratio, fb)
    a = fma(fw[:, 1:2], relw, a)
    a = fma(fw[:, 0:1], relh, a)
    e = _sin_rev(a)                                           # [576, n]
    unf = torch.nn.functional.unfold(x, 3, padding=1).view(b, c * 9, h, w)
    xc = unf[:, :, iy_t][:, :, :, ix_t].reshape(b, c * 9, n)
    xp = e[None] * xc                                         # [b, 576, n], fp32
    wx = torch.cat([get("K.0.0.weight", (HIDDEN, 576))] +
                   [get(f"K.{i}.0.weight", (HIDDEN, HIDDEN + 576))[:, HIDDEN:] for i in (1, 2, 3)], 0)
    bk = torch.cat([get(f"K.{i}.0.bias", (HIDDEN,)) for i in range(4)])[None, :, None]
    q0w, q0b = get("Q.0.0.weight", (HIDDEN, 576)) * inv, get("Q.0.0.bias", (HIDDEN, 1)) * inv
    if arith == "f64":
        pk = wx.double() @ xp.double() + bk.double()
        a0 = q0w.double() @ e.double() + q0b.double()
    else:
        pk = _mm_split(wx, xp) + bk
        a0 = _mm_split(q0w, e) + q0b
    return torch.cat([pk, a0[None].expand(b, HIDDEN, n)], 1).transpose(1, 2).contiguous()


def _initq_forward_split(sd, feat, size, dtype, prefix: str) -> torch.Tensor:
    """``initq_forward_reference(..., split_bf16=True)``: the three split stages -- both planes GEMMs (``initq_planes_reference``),
    and the two 256 x 256 products of layers 1..3 -- with every sine taken of revolutions in float64."""
    dev = feat.device

    def get(name, shape):
        t = sd[prefix + name]
        t = t.detach() if isinstance(t, torch.Tensor) else torch.from_numpy(np.asarray(t))
        return t.to(device=dev, dtype=torch.float32).reshape(shape)

    inv = torch.tensor(INV_2PI_F32, dtype=torch.float32, device=dev)
    hu, wu = int(size[0]), int(size[1])
    pix = initq_planes_reference(sd, feat, size, "split", prefix).transpose(1, 2)      # [b, 1280, n]
    b = pix.shape[0]
    q = torch.relu(pix[:, :HIDDEN]) * _sin_rev(pix[:, P_CHANNELS:])
    for i in (1, 2, 3):
        k = torch.relu(_mm_split(get(f"K.{i}.0.weight", (HIDDEN, HIDDEN + 576))[:, :HIDDEN], q) + pix[:, HIDDEN * i:HIDDEN * (i + 1)])
        s = _mm_split(get(f"Q.{i}.0.weight", (HIDDEN, HIDDEN)) * inv, q) + get(f"Q.{i}.0.bias", (HIDDEN, 1)) * inv
        q = k * _sin_rev(s)
    out = get("last_layer.weight", (3, HIDDEN)) @ q + get("last_layer.bias", (3, 1))
    return out.reshape(b, 3, hu, wu).to(dtype)


def initq_forward_reference(sd, feat, size, dtype=torch.float64, prefix: str = "", planes: Optional[list] = None,
                            split_bf16: bool = False) -> torch.Tensor:
    """The formula sheet of the ``init_q=True``, mode-3 path in tensor algebra, in the RESTRUCTURED form the kernels run
    (any device, any float dtype; the tests' one restatement, as ``encoder_training.rdb_backward_reference`` is for its path).

    Reference (diinn.py:113-115,132-139,163-173), per HR pixel with LR cell (iy, ix)::

        E  = sin(Fw . (rel_h, rel_w, ratio) + Fb)                576 values      first_layer
        x' = E * X[:, iy, ix]                                     X = unfold3x3(feat), index c * 9 + 3 ky + kx, zero padded
        k0 = relu(K0 . x' + bK0);            q0 = k0 * sin(Q0 . E + bQ0)
        k_i = relu(K_i . [q_{i-1}; x'] + bK_i);  q_i = k_i * sin(Q_i . q_{i-1} + bQ_i),  i = 1..3;   out = L . q3 + bL

    Restructured: the feature columns of K_0..3 are stacked into Wx [1024,576], so ``PIX[0:1024] = Wx . x' + bK`` and
    ``PIX[1024:1280] = Q0 . E + bQ0`` are two GEMMs per pixel (``initq_planes_kernel``), and the layers read their seeds
    there: ``k_i = relu(K_i[:, :256] . q_{i-1} + PIX[256 i : 256 i + 256])`` (``decode_kernel<SIN | DECODE_INITQ>``).  E depends on the
    pixel only, not on the batch item.  Coordinates: the fp32 tables of ``axis_tables`` (the reference computes them in fp32
    whatever the module's dtype); ``ratio`` is the Python double rounded to ``dtype``, as ``x.new_tensor`` does.
    ``planes`` (a list): receives every layer's (k_i, s_i), each [B,256,Hu*Wu] -- what the training forward saves.
    ``split_bf16`` (with ``dtype=torch.float32``): the EMULATION of the split-bf16 path (``hip_initq_split_bf16``) -- the two planes
    GEMMs, the ``Q0 . E`` sine argument and layers 1..3 with every operand carried as hi + lo bf16 and a product formed as
    ``(w_lo.x_hi + w_hi.x_lo) + w_hi.x_hi`` in fp32 torch matmuls; sine arguments in revolutions (weights and biases divided by
    fp32(1/(2 pi)) in fp32 before the split, as the images hold them), the sines taken in float64."""
    if split_bf16:
        if dtype != torch.float32 or planes is not None:
            raise ValueError("split_bf16=True emulates fp32 accumulation: dtype=torch.float32, and no planes")
        return _initq_forward_split(sd, feat, size, dtype, prefix)

    def get(name, shape):
        t = sd[prefix + name]
        t = t.detach() if isinstance(t, torch.Tensor) else torch.from_numpy(np.asarray(t))
        return t.to(device=feat.device, dtype=dtype).reshape(shape)

    hu, wu = int(size[0]), int(size[1])
    x = feat.to(dtype)
    b, c, h, w = x.shape
    small = bool(_native.load().diinn_uses_small_output_kernel(hu, wu))
    iy, rel_h = axis_tables(h, hu, small)
    ix, rel_w = axis_tables(w, wu, small)
    dev = feat.device
    iy_t, ix_t = torch.from_numpy(iy.astype(np.int64)).to(dev), torch.from_numpy(ix.astype(np.int64)).to(dev)
    syn = torch.empty((3, hu, wu), dtype=dtype, device=dev)
    syn[0] = torch.from_numpy(rel_h).to(dev, dtype)[:, None]
    syn[1] = torch.from_numpy(rel_w).to(dev, dtype)[None, :]
    syn[2] = torch.tensor((h * w) / (hu * wu), dtype=dtype, device=dev)
    n = hu * wu
    e = torch.sin(get("first_layer.0.weight", (576, 3)) @ syn.reshape(3, n) + get("first_layer.0.bias", (576, 1)))   # [576, n]
    unf = torch.nn.functional.unfold(x, 3, padding=1).view(b, c * 9, h, w)
    xc = unf[:, :, iy_t][:, :, :, ix_t].reshape(b, c * 9, n)
    xp = e[None] * xc                                                                                              # [b, 576, n]
    wx = torch.cat([get("K.0.0.weight", (HIDDEN, 576))] +
                   [get(f"K.{i}.0.weight", (HIDDEN, HIDDEN + 576))[:, HIDDEN:] for i in (1, 2, 3)], 0)          # [1024, 576]
    bk = torch.cat([get(f"K.{i}.0.bias", (HIDDEN,)) for i in range(4)])[None, :, None]
    pix = wx @ xp + bk                                                                                             # [b, 1024, n]
    a0 = get("Q.0.0.weight", (HIDDEN, 576)) @ e + get("Q.0.0.bias", (HIDDEN, 1))                                   # [256, n]
    q = torch.relu(pix[:, :HIDDEN]) * torch.sin(a0)[None]
    if planes is not None:
        planes.append((torch.relu(pix[:, :HIDDEN]), a0[None].expand(b, HIDDEN, n)))
    for i in (1, 2, 3):
        k = torch.relu(get(f"K.{i}.0.weight", (HIDDEN, HIDDEN + 576))[:, :HIDDEN] @ q + pix[:, HIDDEN * i:HIDDEN * (i + 1)])
        s = get(f"Q.{i}.0.weight", (HIDDEN, HIDDEN)) @ q + get(f"Q.{i}.0.bias", (HIDDEN, 1))
        if planes is not None:
            planes.append((k, s))
        q = k * torch.sin(s)
    out = get("last_layer.weight", (3, HIDDEN)) @ q + get("last_layer.bias", (3, 1))
    return out.reshape(b, 3, hu, wu)


def initq_modes_forward_reference(sd, feat, size, mode: int, dtype=torch.float64, prefix: str = "") -> torch.Tensor:
    """The formula sheet of ``init_q=True`` with modes 1, 2 and 4 in tensor algebra, in the RESTRUCTURED form the kernels run (any
    device, any float dtype), beside ``initq_forward_reference`` (mode 3).

    Reference (diinn.py:112-147), per HR pixel: ``E`` and ``x' = E * X[cell]`` as for mode 3, ``k0 = relu(K0 . x' + bK0)``,
    ``q0 = k0 * sin(Q0 . E + bQ0)``, ``q_i = k_i * sin(Q_i . q_{i-1} + bQ_i)`` and

        mode 1   k_i = relu(K_i . k_{i-1} + bK_i)            K_i [256,256]
        mode 2   k_i = relu(K_i . [k_{i-1}; x'] + bK_i)      K_i [256,832]
        mode 4   k_i = relu(K_i . [q_{i-1}; x'] + bK_i),     then Conv2d(256, 3, 3, padding=1, 'reflect') over the HR grid

    Restructured, with the pixel record ``PIX`` of ``initq_forward_reference``:

        modes 1/2  PIX[0:256] = K0 . x' + bK0, PIX[1024:1280] = Q0 . E + bQ0 (mode 1: these 512 rows are the whole GEMM,
                   ``initq_planes_kernel<SIN | INITQ_ROWS512>``); PIX[256 i : 256 i + 256] = K_i[:, 256:] . x' + bK_i (mode 2) or the seed
                   is bK_i itself (mode 1).  The chain ``k_i = relu(K_i[:, :256] . k_{i-1} + seed_i)`` runs per pixel on its own
                   (``pixel_chain_kernel``) and the layers read it as the multiplier (``decode_kernel<SIN | DECODE_INITQ, KPART=false>``).
        mode 4     mode 3's layers from the 1280-row record, the head as 27 tap values per pixel, T[3 ky + kx][c] =
                   Lw[c, :, ky, kx] . q3 (``decode_kernel<SIN | DECODE_INITQ | DECODE_TAPS>``), and the reflect-padded 9-point gather
                   over the image (``head3x3_reflect_kernel``).
    Coordinates and ``ratio`` as in ``initq_forward_reference``."""
    if mode not in (1, 2, 4):
        raise ValueError(f"initq_modes_forward_reference states modes 1, 2 and 4 (mode 3: initq_forward_reference), got {mode}")

    def get(name, shape):
        t = sd[prefix + name]
        t = t.detach() if isinstance(t, torch.Tensor) else torch.from_numpy(np.asarray(t))
        return t.to(device=feat.device, dtype=dtype).reshape(shape)

    hu, wu = int(size[0]), int(size[1])
    x = feat.to(dtype)
    b, c, h, w = x.shape
    small = bool(_native.load().diinn_uses_small_output_kernel(hu, wu))
    iy, rel_h = axis_tables(h, hu, small)
    ix, rel_w = axis_tables(w, wu, small)
    dev = feat.device
    iy_t, ix_t = torch.from_numpy(iy.astype(np.int64)).to(dev), torch.from_numpy(ix.astype(np.int64)).to(dev)
    syn = torch.empty((3, hu, wu), dtype=dtype, device=dev)
    syn[0] = torch.from_numpy(rel_h).to(dev, dtype)[:, None]
    syn[1] = torch.from_numpy(rel_w).to(dev, dtype)[None, :]
    syn[2] = torch.tensor((h * w) / (hu * wu), dtype=dtype, device=dev)
    n = hu * wu
    e = torch.sin(get("first_layer.0.weight", (576, 3)) @ syn.reshape(3, n) + get("first_layer.0.bias", (576, 1)))   # [576, n]
    unf = torch.nn.functional.unfold(x, 3, padding=1).view(b, c * 9, h, w)
    xp = e[None] * unf[:, :, iy_t][:, :, :, ix_t].reshape(b, c * 9, n)                                               # [b, 576, n]
    kin = HIDDEN if mode == 1 else HIDDEN + 576
    kw = [get(f"K.{i}.0.weight", (HIDDEN, kin)) for i in (1, 2, 3)]
    bk = [get(f"K.{i}.0.bias", (HIDDEN, 1)) for i in range(4)]
    k = torch.relu(get("K.0.0.weight", (HIDDEN, 576)) @ xp + bk[0])                                                 # PIX[0:256]
    q = k * torch.sin(get("Q.0.0.weight", (HIDDEN, 576)) @ e + get("Q.0.0.bias", (HIDDEN, 1)))[None]              # PIX[1024:1280]
    for i in (1, 2, 3):
        seed = bk[i] if mode == 1 else kw[i - 1][:, HIDDEN:] @ xp + bk[i]                                         # PIX[256 i : 256 i + 256]
        k = torch.relu(kw[i - 1][:, :HIDDEN] @ (q if mode == 4 else k) + seed)
        q = k * torch.sin(get(f"Q.{i}.0.weight", (HIDDEN, HIDDEN)) @ q + get(f"Q.{i}.0.bias", (HIDDEN, 1)))
    if mode != 4:
        return (get("last_layer.weight", (3, HIDDEN)) @ q + get("last_layer.bias", (3, 1))).reshape(b, 3, hu, wu)
    lw = get("last_layer.weight", (3, HIDDEN, 3, 3))
    taps = torch.einsum("chyx,bhn->byxcn", lw, q).reshape(b, 3, 3, 3, hu, wu)                                     # T[ky][kx][c] per pixel
    ry = torch.arange(-1, hu + 1, device=dev).abs()
    ry = torch.where(ry >= hu, 2 * (hu - 1) - ry, ry)                                                              # 'reflect': -1 -> 1, Hu -> Hu - 2
    rx = torch.arange(-1, wu + 1, device=dev).abs()
    rx = torch.where(rx >= wu, 2 * (wu - 1) - rx, rx)
    out = get("last_layer.bias", (1, 3, 1, 1)).expand(b, 3, hu, wu).clone()
    for ky in range(3):
        for kx in range(3):
            out = out + taps[:, ky, kx][:, :, ry[ky:ky + hu]][:, :, :, rx[kx:kx + wu]]
    return out


def modes_x3_forward_reference(sd, feat, size, mode: int, prefix: str = "") -> torch.Tensor:
    """The EMULATION sheet of the split-bf16 arithmetic of decoder modes 1, 2 and 4 with ``init_q=False``
    (``decode_features(..., compute="bf16x3", modes_x3=True)``), in fp32 torch algebra on any device; beside
    ``initq_forward_reference(..., split_bf16=True)``, which states mode 3 with ``init_q=True``.

    What is split: the three synthesis products ``Q_i . q_{i-1}``, i = 1..3, of every mode, and for mode 4 the three modulation
    products ``K_i[:, :256] . q_{i-1}`` as well.  Every operand of such a product is carried as hi = bf16(v), lo = bf16(v - hi) and
    the product formed as ``(w_lo.q_hi + w_hi.q_lo) + w_hi.q_hi`` in fp32 (``_mm_split``: torch matmuls, not the MFMA's summation
    order).  The synthesis branch runs in REVOLUTIONS: Q_0..3 and their biases are multiplied by fp32(1/(2 pi)) in fp32 before the
    split, as the body image holds them, and every sine is taken of revolutions in float64 (``_sin_rev``).

    What stays fp32: the hoisted conv ``P = Wx . unfold3x3(feat) + bK`` (mode 1: ``P_i = bK_i`` for i >= 1), the per-cell
    modulation chain of modes 1/2, ``k_0 = relu(P_0)``, ``k_i = relu(K_i[:, :256] . k_{i-1} + P_i)`` (``cell_chain_kernel``), layer
    0 with the kernels' fma sequence ``a = fma(Q0_h, rel_h, fma(Q0_w, rel_w, fma(Q0_r, ratio, bQ0)))``, the seeds and biases, and
    the head on the unsplit ``q_3``: ``L . q_3 + bL`` (modes 1/2), or the 27 tap values per pixel and the reflect-padded 9-point
    gather (mode 4)."""
    if mode not in (1, 2, 4):
        raise ValueError(f"modes_x3_forward_reference states modes 1, 2 and 4, got {mode}")
    f32 = torch.float32
    dev = feat.device

    def get(name, shape):
        t = sd[prefix + name]
        t = t.detach() if isinstance(t, torch.Tensor) else torch.from_numpy(np.asarray(t))
        return t.to(device=dev, dtype=f32).reshape(shape)

    def fma(a_, b_, c_):                                      # one rounding: the fp32 product is exact in float64
        return (a_.double() * b_.double() + c_.double()).to(f32)

    inv = torch.tensor(INV_2PI_F32, dtype=f32, device=dev)
    hu, wu = int(size[0]), int(size[1])
    x = feat.to(f32)
    b, c, h, w = x.shape
    n = hu * wu
    small = bool(_native.load().diinn_uses_small_output_kernel(hu, wu))
    iy, rel_h = axis_tables(h, hu, small)
    ix, rel_w = axis_tables(w, wu, small)
    iy_t, ix_t = torch.from_numpy(iy.astype(np.int64)).to(dev), torch.from_numpy(ix.astype(np.int64)).to(dev)
    relh = torch.from_numpy(rel_h).to(dev, f32)[:, None].expand(hu, wu).reshape(1, n)
    relw = torch.from_numpy(rel_w).to(dev, f32)[None, :].expand(hu, wu).reshape(1, n)
    ratio = torch.tensor(np.float32((h * w) / (hu * wu)), dtype=f32, device=dev)
    kin = HIDDEN if mode == 1 else HIDDEN + 576
    kw = [get(f"K.{i}.0.weight", (HIDDEN, kin)) for i in (1, 2, 3)]
    bk = [get(f"K.{i}.0.bias", (HIDDEN, 1)) for i in range(4)]
    unf = torch.nn.functional.unfold(x, 3, padding=1)                                   # [b, 576, h*w], fp32
    P = [get("K.0.0.weight", (HIDDEN, 576)) @ unf + bk[0]]
    for i in (1, 2, 3):
        P.append(bk[i].expand(b, HIDDEN, h * w) if mode == 1 else kw[i - 1][:, HIDDEN:] @ unf + bk[i])
    cell = (iy_t[:, None] * w + ix_t[None, :]).reshape(n)                               # LR cell of every HR pixel
    if mode != 4:                                                                       # the per-cell chain, fp32
        kc = [torch.relu(P[0])]
        for i in (1, 2, 3):
            kc.append(torch.relu(kw[i - 1][:, :HIDDEN] @ kc[-1] + P[i]))
    q0w, q0b = get("Q.0.0.weight", (HIDDEN, 3)) * inv, get("Q.0.0.bias", (HIDDEN, 1)) * inv
    a = fma(q0w[:, 2:3], ratio, q0b)
    a = fma(q0w[:, 1:2], relw, a)
    a = fma(q0w[:, 0:1], relh, a)
    q = torch.relu(P[0][:, :, cell]) * _sin_rev(a)[None]                                # [b, 256, n]
    for i in (1, 2, 3):
        s = _mm_split(get(f"Q.{i}.0.weight", (HIDDEN, HIDDEN)) * inv, q) + get(f"Q.{i}.0.bias", (HIDDEN, 1)) * inv
        if mode == 4:
            k = torch.relu(_mm_split(kw[i - 1][:, :HIDDEN], q) + P[i][:, :, cell])
        else:
            k = kc[i][:, :, cell]
        q = k * _sin_rev(s)
    if mode != 4:
        return (get("last_layer.weight", (3, HIDDEN)) @ q + get("last_layer.bias", (3, 1))).reshape(b, 3, hu, wu)
    lw = get("last_layer.weight", (3, HIDDEN, 3, 3))
    taps = torch.einsum("chyx,bhn->byxcn", lw, q).reshape(b, 3, 3, 3, hu, wu)           # T[ky][kx][c] per pixel
    ry = torch.arange(-1, hu + 1, device=dev).abs()
    ry = torch.where(ry >= hu, 2 * (hu - 1) - ry, ry)                                    # 'reflect': -1 -> 1, Hu -> Hu - 2
    rx = torch.arange(-1, wu + 1, device=dev).abs()
    rx = torch.where(rx >= wu, 2 * (wu - 1) - rx, rx)
    out = get("last_layer.bias", (1, 3, 1, 1)).expand(b, 3, hu, wu).clone()
    for ky in range(3):
        for kx in range(3):
            out = out + taps[:, ky, kx][:, :, ry[ky:ky + hu]][:, :, :, rx[kx:kx + wu]]
    return out


def mode4_rows(h: int, hu: int, wu: int, y0: int, y1: int) -> Tuple[Tuple[int, int], Tuple[int, int]]:
    """((ty0, ty1), (r0, r1)): the HR rows whose tap values mode 4 needs for output rows [y0,y1) (one more row each way,
    clipped to the image) and the LR rows those read (C ABI ``diinn_mode4_rows``)."""
    lib = _native.load()
    a, b, r0, r1 = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    _native.check(lib.diinn_mode4_rows(h, hu, wu, y0, y1, C.byref(a), C.byref(b), C.byref(r0), C.byref(r1)),
                  "diinn_mode4_rows")
    return (a.value, b.value), (r0.value, r1.value)


def axis_tables(n_in: int, n_out: int, small_output: bool = False) -> Tuple[np.ndarray, np.ndarray]:
    """Host tables (idx int32, rel fp32) from the C ABI ``diinn_make_axis_tables``."""
    lib = _native.load()
    idx = np.empty(n_out, np.int32)
    rel = np.empty(n_out, np.float32)
    st = lib.diinn_make_axis_tables(n_in, n_out, int(small_output),
                                    idx.ctypes.data_as(_native._i32), _native.fptr(rel))
    _native.check(st, "diinn_make_axis_tables")
    return idx, rel


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
    if feat.dtype != torch.float32 or feat.dim() != 4 or feat.shape[1] != IN_CHANNELS:
        raise ValueError(f"feat must be fp32 [B,{IN_CHANNELS},H,W], got {feat.dtype} {tuple(feat.shape)}")
    hu, wu = size  # same unpack as the reference (diinn.py:96): raises unless len(size) == 2
    hu, wu = int(hu), int(wu)
    feat = feat.contiguous()
    b, _, h, w = feat.shape
    y0, y1 = (0, hu) if rows is None else (int(rows[0]), int(rows[1]))
    if out is None:
        out = torch.empty((b, 3, hu, wu), dtype=torch.float32, device=feat.device)
    else:
        if out.shape != (b, 3, hu, wu) or out.dtype != torch.float32 or not out.is_contiguous() \
                or out.device != feat.device:
            raise ValueError("out must be a contiguous fp32 [B,3,Hu,Wu] tensor on feat's device")
    if initq is not None:
        _require_cuda(initq, "init_q image")
        pneed = lib.diinn_initq_pix_bytes(b, wu, y1 - y0)
        if pneed == 0 or y0 < 0 or y1 > hu:
            raise ValueError(f"rows {(y0, y1)} are not a band of an image of {hu} rows")
        if pix is None:
            pix = torch.empty(pneed // 4, dtype=torch.float32, device=feat.device)
        elif pix.numel() * pix.element_size() < pneed or pix.dtype != torch.float32 or not pix.is_contiguous() \
                or pix.device != feat.device:
            raise ValueError(f"pix must be a contiguous fp32 buffer of >= {pneed} bytes on feat's device")
        if initq_x3 is not None:
            _require_cuda(initq_x3, "init_q split image")
            with torch.cuda.device(feat.device):
                stream = torch.cuda.current_stream().cuda_stream
                st = lib.diinn_decode_initq_x3(C.c_void_p(stream), C.c_void_p(feat.data_ptr()), C.c_void_p(packed.data_ptr()),
                                               C.c_void_p(initq.data_ptr()), C.c_void_p(initq_x3.data_ptr()),
                                               C.c_void_p(pix.data_ptr()), C.c_void_p(out.data_ptr()),
                                               b, h, w, hu, wu, y0, y1, int(sin_mode))
            _native.check(st, "diinn_decode_initq_x3")
            return out
        with torch.cuda.device(feat.device):
            stream = torch.cuda.current_stream().cuda_stream
            st = lib.diinn_decode_initq(C.c_void_p(stream), C.c_void_p(feat.data_ptr()), C.c_void_p(packed.data_ptr()),
                                        C.c_void_p(initq.data_ptr()), C.c_void_p(pix.data_ptr()), C.c_void_p(out.data_ptr()),
                                        b, h, w, hu, wu, y0, y1, int(sin_mode))
        _native.check(st, "diinn_decode_initq")
        return out
    need = lib.diinn_workspace_bytes(b, h, w)
    if workspace is None:
        workspace = torch.empty(need // 4, dtype=torch.float32, device=feat.device)
    elif workspace.numel() * workspace.element_size() < need or not workspace.is_contiguous() \
            or workspace.device != feat.device:
        raise ValueError(f"workspace must be a contiguous buffer of >= {need} bytes on feat's device")
    if mode not in (1, 2, 3, 4):
        raise NotImplementedError(f"mode {mode}: the HIP path covers modes 1-4")
    x3 = bool(modes_x3) and mode != 3 and compute == "bf16x3"     # the opt-in: split bf16 for modes 1, 2 and 4
    if mode != 3 and compute != "f32" and not x3:
        raise ValueError("modes 1, 2 and 4 run in fp32 only")
    if mode == 4:
        if head is None:
            raise ValueError("mode 4 needs its 3x3 head image: head=pack_head3x3(state_dict) on feat's device")
        _require_cuda(head, "head image")
        if hu < 2 or wu < 2:
            raise ValueError(f"mode 4: the reflect-padded 3x3 head needs an output of at least 2 x 2, got {hu} x {wu}")
        tneed = lib.diinn_mode4_taps_bytes(b, hu, wu, y0, y1)
        if tneed == 0:
            raise ValueError(f"rows {(y0, y1)} are not a band of an image of {hu} rows")
        if taps is None:
            taps = torch.empty(tneed // 4, dtype=torch.float32, device=feat.device)
        elif taps.numel() * taps.element_size() < tneed or not taps.is_contiguous() or taps.device != feat.device:
            raise ValueError(f"taps must be a contiguous buffer of >= {tneed} bytes on feat's device")
        name = "diinn_decode_mode4_x3" if x3 else "diinn_decode_mode4"
        with torch.cuda.device(feat.device):
            stream = torch.cuda.current_stream().cuda_stream
            st = getattr(lib, name)(C.c_void_p(stream), C.c_void_p(feat.data_ptr()), C.c_void_p(packed.data_ptr()),
                                    C.c_void_p(head.data_ptr()), C.c_void_p(workspace.data_ptr()),
                                    C.c_void_p(taps.data_ptr()), C.c_void_p(out.data_ptr()),
                                    b, h, w, hu, wu, y0, y1, int(sin_mode))
        _native.check(st, name)
        return out
    comp = _native.COMPUTE[compute] if mode == 3 else _native.COMPUTE_F32_QONLY
    with torch.cuda.device(feat.device):
        stream = torch.cuda.current_stream().cuda_stream
        if x3:
            st = lib.diinn_decode_qonly_x3(C.c_void_p(stream), C.c_void_p(feat.data_ptr()), C.c_void_p(packed.data_ptr()),
                                           C.c_void_p(workspace.data_ptr()), C.c_void_p(out.data_ptr()),
                                           b, h, w, hu, wu, y0, y1, int(sin_mode))
            _native.check(st, "diinn_decode_qonly_x3")
            return out
        st = lib.diinn_decode_ex(C.c_void_p(stream), C.c_void_p(feat.data_ptr()), C.c_void_p(packed.data_ptr()),
                                 C.c_void_p(workspace.data_ptr()), C.c_void_p(out.data_ptr()),
                                 b, h, w, hu, wu, y0, y1, int(sin_mode), comp)
    _native.check(st, "diinn_decode_ex")
    return out


def decode_features_initq(feat: torch.Tensor, packed: torch.Tensor, initq: torch.Tensor, size: Sequence[int], mode: int,
                          head: Optional[torch.Tensor] = None, taps: Optional[torch.Tensor] = None,
                          pix: Optional[torch.Tensor] = None, rows: Optional[Tuple[int, int]] = None,
                          out: Optional[torch.Tensor] = None, sin_mode: int = _native.SIN_DEFAULT,
                          planes_rows: Optional[int] = None) -> torch.Tensor:
    """``init_q=True`` with decoder modes 1, 2 and 4 (fp32, inference): encoder features ``feat`` [B,64,H,W] -> RGB [B,3,Hu,Wu].
    (Mode 3 is ``decode_features(..., initq=...)``, which keeps refusing these modes.)

    ``packed`` = ``pack_state_dict(initq_body_state_dict(sd), mode=mode)``, ``initq`` = ``pack_initq(sd)``, ``head`` (mode 4) =
    ``pack_head3x3(sd)``, all on feat's device.  ``rows=(y0,y1)`` computes only that HR row band, bit-identical to the same rows
    of a whole-image decode; the rest of ``out`` is left untouched.  ``pix``: the pixel planes, 5,120 bytes per HR pixel of the
    rows decoded -- for mode 4 of the tap rows [max(0, y0-1), min(Hu, y1+1)) (``diinn_initq_mode4_pix_bytes``), as is ``taps``
    (``diinn_mode4_taps_bytes``); both allocated if None.  ``planes_rows`` (mode 1): 512 (default; the planes kernel computes the 512
    GEMM rows mode 1 has, the chain takes its seeds from the biases) or 1280 (mode 2's form on the zero-widened image: the
    same bits).  Enqueues three kernels on the current stream; never synchronises."""
    lib = _native.load()
    if mode not in (1, 2, 4):
        raise NotImplementedError(f"decode_features_initq covers modes 1, 2 and 4 (mode 3: decode_features(..., initq=...)), got mode {mode}")
    if planes_rows not in ((None, 512, 1280) if mode == 1 else (None, 1280)):
        raise ValueError(f"planes_rows={planes_rows}: mode 1 takes 512 or 1280, modes 2 and 4 the 1280-row planes only")
    _require_cuda(feat, "feat")
    _require_cuda(packed, "packed weights")
    _require_cuda(initq, "init_q image")
    if feat.dtype != torch.float32 or feat.dim() != 4 or feat.shape[1] != IN_CHANNELS:
        raise ValueError(f"feat must be fp32 [B,{IN_CHANNELS},H,W], got {feat.dtype} {tuple(feat.shape)}")
    hu, wu = size
    hu, wu = int(hu), int(wu)
    feat = feat.contiguous()
    b, _, h, w = feat.shape
    y0, y1 = (0, hu) if rows is None else (int(rows[0]), int(rows[1]))
    if mode == 4:
        if head is None:
            raise ValueError("mode 4 needs its 3x3 head image: head=pack_head3x3(state_dict) on feat's device")
        _require_cuda(head, "head image")
        if hu < 2 or wu < 2:
            raise ValueError(f"mode 4: the reflect-padded 3x3 head needs an output of at least 2 x 2, got {hu} x {wu}")
    if out is None:
        out = torch.empty((b, 3, hu, wu), dtype=torch.float32, device=feat.device)
    elif out.shape != (b, 3, hu, wu) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != feat.device:
        raise ValueError("out must be a contiguous fp32 [B,3,Hu,Wu] tensor on feat's device")
    pneed = lib.diinn_initq_mode4_pix_bytes(b, hu, wu, y0, y1) if mode == 4 else \
        (lib.diinn_initq_pix_bytes(b, wu, y1 - y0) if 0 <= y0 < y1 <= hu else 0)
    if pneed == 0:
        raise ValueError(f"rows {(y0, y1)} are not a band of an image of {hu} rows")
    if pix is None:
        pix = torch.empty(pneed // 4, dtype=torch.float32, device=feat.device)
    elif pix.numel() * pix.element_size() < pneed or pix.dtype != torch.float32 or not pix.is_contiguous() \
            or pix.device != feat.device:
        raise ValueError(f"pix must be a contiguous fp32 buffer of >= {pneed} bytes on feat's device")
    ptr = lambda t: C.c_void_p(t.data_ptr())
    with torch.cuda.device(feat.device):
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        if mode == 4:
            tneed = lib.diinn_mode4_taps_bytes(b, hu, wu, y0, y1)
            if taps is None:
                taps = torch.empty(tneed // 4, dtype=torch.float32, device=feat.device)
            elif taps.numel() * taps.element_size() < tneed or not taps.is_contiguous() or taps.device != feat.device:
                raise ValueError(f"taps must be a contiguous buffer of >= {tneed} bytes on feat's device")
            name = "diinn_decode_initq_mode4"
            st = lib.diinn_decode_initq_mode4(stream, ptr(feat), ptr(packed), ptr(initq), ptr(head), ptr(pix), ptr(taps), ptr(out),
                                              b, h, w, hu, wu, y0, y1, int(sin_mode))
        else:
            name = "diinn_decode_initq_mode1" if mode == 1 and planes_rows != 1280 else "diinn_decode_initq_mode2"
            st = getattr(lib, name)(stream, ptr(feat), ptr(packed), ptr(initq), ptr(pix), ptr(out),
                                    b, h, w, hu, wu, y0, y1, int(sin_mode))
    _native.check(st, name)
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
    lib = _native.load()
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
    (_, _), (r0, rn) = window_rows(int(full_h), hu, wu, y0, y1)
    need = b * rn * w * P_CHANNELS
    if p_win is None:
        p_win = torch.empty(need, dtype=torch.float32, device=feat_win.device)
    elif p_win.numel() < need or p_win.dtype != torch.float32 or not p_win.is_contiguous() \
            or p_win.device != feat_win.device:
        raise ValueError(f"p_win must be a contiguous fp32 buffer of >= {need} floats on feat_win's device")
    if out_win is None:
        out_win = torch.empty((b, 3, y1 - y0, wu), dtype=torch.float32, device=feat_win.device)
    elif out_win.shape != (b, 3, y1 - y0, wu) or out_win.dtype != torch.float32 or not out_win.is_contiguous() \
            or out_win.device != feat_win.device:
        raise ValueError("out_win must be a contiguous fp32 [B,3,y1-y0,Wu] tensor on feat_win's device")
    if mode not in (1, 2, 3):
        raise NotImplementedError(f"mode {mode}: windows and tiles cover modes 1-3 (mode 4's 3x3 head reads its "
                                  f"neighbours' rows and columns: decode it with decode_features(rows=...))")
    if mode != 3 and compute != "f32":
        raise ValueError("modes 1 and 2 run in fp32 only")
    comp = _native.COMPUTE[compute] if mode == 3 else _native.COMPUTE_F32_QONLY
    with torch.cuda.device(feat_win.device):
        stream = torch.cuda.current_stream().cuda_stream
        st = lib.diinn_decode_win(C.c_void_p(stream), C.c_void_p(feat_win.data_ptr()), int(feat_row0), fr,
                                  C.c_void_p(packed.data_ptr()), C.c_void_p(p_win.data_ptr()), r0, rn,
                                  C.c_void_p(out_win.data_ptr()), y0, y1 - y0,
                                  b, int(full_h), w, hu, wu, y0, y1, int(sin_mode), comp)
    _native.check(st, "diinn_decode_win")
    return out_win


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
    lib = _native.load()
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
    p_rows = p_win.numel() // (b * w * P_CHANNELS)
    if mode not in (1, 2, 3):
        raise NotImplementedError(f"mode {mode}: windows and tiles cover modes 1-3 (mode 4's 3x3 head reads its "
                                  f"neighbours' rows and columns: decode it with decode_features(rows=...))")
    if mode != 3 and compute != "f32":
        raise ValueError("modes 1 and 2 run in fp32 only")
    comp = _native.COMPUTE[compute] if mode == 3 else _native.COMPUTE_F32_QONLY
    with torch.cuda.device(p_win.device):
        stream = torch.cuda.current_stream().cuda_stream
        st = lib.diinn_decode_tile_win(C.c_void_p(stream), C.c_void_p(p_win.data_ptr()), int(p_row0), p_rows,
                                       C.c_void_p(packed.data_ptr()), C.c_void_p(out.data_ptr()),
                                       out.stride(2), out.stride(1), out.stride(0), b, h, w, hu, wu, y0, y1, x0, x1,
                                       int(sin_mode), comp)
    _native.check(st, "diinn_decode_tile_win")
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


def _comparison_decode(fn, fn_name: str, workspace_bytes, feat: torch.Tensor, packed: torch.Tensor, size: Sequence[int],
                       out: Optional[torch.Tensor], workspace: Optional[torch.Tensor]) -> torch.Tensor:
    """The LIIF / MetaSR decode of every HR pixel: ``fn`` (a library entry point with diinn_liif_decode's signature, ``fn_name`` for
    the error message) with ``workspace_bytes(B, H, W)`` bytes of workspace; a ``workspace`` that is too small is replaced."""
    _require_cuda(feat, "feat")
    _require_cuda(packed, "packed weights")
    if feat.dtype != torch.float32 or feat.dim() != 4 or feat.shape[1] != IN_CHANNELS:
        raise ValueError(f"feat must be fp32 [B,{IN_CHANNELS},H,W], got {feat.dtype} {tuple(feat.shape)}")
    hu, wu = size
    hu, wu = int(hu), int(wu)
    feat = feat.contiguous()
    b, _, h, w = feat.shape
    if out is None:
        out = torch.empty((b, 3, hu, wu), dtype=torch.float32, device=feat.device)
    elif out.shape != (b, 3, hu, wu) or out.dtype != torch.float32 or not out.is_contiguous() \
            or out.device != feat.device:
        raise ValueError("out must be a contiguous fp32 [B,3,Hu,Wu] tensor on feat's device")
    need = workspace_bytes(b, h, w)
    if workspace is None or workspace.numel() * 4 < need or workspace.device != feat.device:
        workspace = torch.empty(need // 4, dtype=torch.float32, device=feat.device)
    with torch.cuda.device(feat.device):
        stream = torch.cuda.current_stream().cuda_stream
        st = fn(C.c_void_p(stream), C.c_void_p(feat.data_ptr()), C.c_void_p(packed.data_ptr()),
                C.c_void_p(workspace.data_ptr()), C.c_void_p(out.data_ptr()), b, h, w, hu, wu)
    _native.check(st, fn_name)
    return out


def liif_decode_features(feat: torch.Tensor, packed: torch.Tensor, size: Sequence[int],
                         out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """LIIF query of every HR pixel: encoder features [B,64,H,W] -> RGB [B,3,Hu,Wu] (liif.py:59-127,148-155)."""
    lib = _native.load()
    return _comparison_decode(lib.diinn_liif_decode, "diinn_liif_decode", lib.diinn_workspace_bytes, feat, packed, size, out, workspace)


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
    lib = _native.load()
    return _comparison_decode(lib.diinn_metasr_decode, "diinn_metasr_decode", lib.diinn_metasr_workspace_bytes, feat, packed, size, out,
                              workspace)


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

    ``hip_autograd`` (a plain attribute, also a constructor keyword; default False) opts ``init_q=True``, mode 3, fp32 into
    training: with it set, ``forward(x, size, None)`` under autograd runs ``initq_training.DecodeInitqFunction`` (the HIP kernels
    saving the activations, the backward pass on the HIP kernels; ROCm GPU only).  With ``bsize`` given the call stays the no_grad
    inference path, like the reference's ``batched_step``.  It changes nothing else: modes 1, 2 and 4 with ``init_q``, the bf16
    arithmetics and every decoder with ``init_q=False`` behave as without it.

    ``hip_autograd_mode4`` (a plain attribute, also a constructor keyword; default False) opts mode 4, ``init_q=False``, fp32 into
    training: with it set, ``forward(x, size, None)`` under autograd runs ``mode4_training.DecodeMode4Function`` (mode 3's training
    forward for the saved activations, the 3x3 head from those planes, the backward pass on the HIP kernels; ROCm GPU only, the
    output at least 2 x 2).  With ``bsize`` given the call stays the no_grad inference path.  It changes nothing else:
    ``hip_autograd`` alone does not open mode 4, and mode 4 with ``init_q=True`` or a bf16 arithmetic keeps refusing.

    ``hip_initq_modes`` (a plain attribute, also a constructor keyword; default False) opts ``init_q=True`` with modes 1, 2 and 4
    into INFERENCE on the HIP path (fp32; ``decode_features_initq``: the per-pixel modulation chain of modes 1/2, mode 4's tap form
    on the pixel planes).  With it unset those decoders refuse exactly as before.  With it set they still
    refuse autograd (``hip_autograd`` / ``hip_autograd_mode4`` do not open it; ``hip_autograd_initq_modes``, below, does), the bf16 arithmetics, ``DIINN(graphs=True)`` and the
    sharded forward; it changes nothing for mode 3 or ``init_q=False``.

    ``hip_initq_split_bf16`` (a plain attribute, also a constructor keyword; default False) opts ``init_q=True``, mode 3, INFERENCE
    into ``compute="bf16x3"``, the split-bf16 arithmetic (``initq_planes_x3_kernel`` and the init_q form of ``decode_bf16x3_kernel``;
    DESIGN.md 3.6d).  With it unset every ``compute`` other than ``"f32"`` refuses as before.  With it set only ``"bf16x3"`` opens:
    ``"bf16"`` / ``"bf16_full"``, autograd, ``init_q`` with modes 1/2/4, ``DIINN(graphs=True)`` and the sharded forward keep
    refusing with their messages, and ``compute="f32"`` gives the fp32 bits.  ``DIINN.set_split_bf16()`` does not set it: on an
    ``init_q`` model the user sets both.

    ``hip_autograd_initq_modes`` (a plain attribute, also a constructor keyword; default False) opts ``init_q=True`` with modes 1, 2
    and 4 into TRAINING, and acts only together with ``hip_initq_modes``, in fp32: with both set, ``forward(x, size, None)`` under
    autograd runs ``initq_modes_training.DecodeInitqModesFunction`` (modes 1/2: the per-pixel modulation chain forwards and, on
    pixel_chain_bwd_kernel, backwards; mode 4: mode 3's ``init_q`` training forward, the 3x3 head from its saved planes, the output
    at least 2 x 2; ROCm GPU only).  With ``bsize`` given or under ``no_grad`` the call is ``hip_initq_modes``'
    inference path, bit for bit.  Set alone it changes nothing; with it unset every call refuses as before (``hip_autograd`` and
    ``hip_autograd_mode4`` still do not open these combinations); the bf16 arithmetics, ``DIINN(graphs=True)`` and the sharded
    forward keep refusing.

    ``hip_autograd_split_bf16`` (a plain attribute, also a constructor keyword; default False) opts mode 3, ``init_q=False``,
    ``compute="bf16x3"`` into TRAINING: with it set, ``forward(x, size, None)`` under autograd runs
    ``split_training.DecodeMode3SplitFunction`` -- the per-pixel chain in split-bf16 arithmetic forwards
    (``decode_bf16x3_kernel<SAVE>``) and backwards (``bwd_layer_x3_kernel``), everything else of the step the fp32 kernels
    (ROCm GPU only).  It acts for no other combination: with it unset every call refuses or runs exactly as
    before; with it set modes 1, 2, 4 and ``init_q=True`` with ``compute="bf16x3"`` under autograd, ``"bf16"`` and
    ``"bf16_full"`` under autograd, ``DIINN(graphs=True)`` and the sharded forward keep refusing, and ``compute="f32"`` trains in
    fp32 as always.  ``DIINN.set_split_bf16()`` does not set it: a user who wants to train in the split arithmetic sets both.

    ``hip_modes_split_bf16`` (a plain attribute, also a constructor keyword; default False) opts modes 1, 2 and 4, ``init_q=False``,
    INFERENCE into ``compute="bf16x3"``: with it set, ``forward`` under ``no_grad`` (or with ``bsize`` given) runs
    ``decode_features(..., compute="bf16x3", modes_x3=True)`` -- the Q-only form of ``decode_bf16x3_kernel`` for modes 1/2, its tap
    form for mode 4 (chunked by ``MODE4_CHUNK_ROWS`` like the fp32 path; ``DIINN(graphs=True)`` replays it) -- DESIGN.md 3.5b.  With
    it unset these modes refuse every ``compute`` but ``"f32"`` as before.  With it set the following keep refusing with their
    messages: autograd through these modes with ``"bf16x3"``; ``init_q=True`` with modes 1/2/4 in any bf16 arithmetic;
    ``DIINN.forward_sharded``; ``"bf16"`` and ``"bf16_full"``.  It changes nothing for mode 3 or for ``compute="f32"``.
    ``DIINN.set_split_bf16()`` does not set it: on such a model the user sets both."""

    hip_autograd = False
    hip_autograd_mode4 = False
    hip_initq_modes = False
    hip_initq_split_bf16 = False
    hip_autograd_initq_modes = False
    hip_autograd_split_bf16 = False
    hip_modes_split_bf16 = False

    def __init__(self, in_channels: int = 64, hidden_dims=(256, 256, 256, 256), mode: int = 1,
                 init_q: bool = False, sin_mode: int = _native.SIN_DEFAULT, compute: str = "f32", hip_autograd: bool = False,
                 hip_autograd_mode4: bool = False, hip_initq_modes: bool = False, hip_initq_split_bf16: bool = False,
                 hip_autograd_initq_modes: bool = False, hip_autograd_split_bf16: bool = False,
                 hip_modes_split_bf16: bool = False):
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

    def _initq_modes(self) -> bool:
        """``init_q=True`` with mode 1, 2 or 4 and the opt-in set: the paths of ``decode_features_initq``."""
        return bool(self.init_q and self.hip_initq_modes and self.mode in (1, 2, 4))

    def _check_supported(self):
        if self.mode not in (1, 2, 3, 4) or (self.init_q and self.mode != 3 and not self._initq_modes()):
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

        ``init_q=True`` with modes 1, 2, 4 (``hip_initq_modes`` set; fp32, inference only): the same chunks of HR rows; mode 4
        computes the planes and the taps of a chunk's rows plus one row each way, clipped to the image, and it is those
        ``initq_chunk_rows`` rows that stay within the cap (a chunk is two output rows shorter).  Chunks change no bit,
        ``bsize`` is ignored, and mode 4 reproduces ``bsize=None`` as it does without ``init_q``.  Under autograd with ``bsize=None``
        it raises unless ``hip_autograd_initq_modes`` is set as well (then: ``initq_modes_training.DecodeInitqModesFunction``, the
        whole image at once)."""
        self._check_supported()
        wants_grad = bsize is None and torch.is_grad_enabled() and (
            x.requires_grad or any(p.requires_grad for p in self.parameters()))
        # the opt-in (initq_modes_training.py): acts only together with hip_initq_modes, in fp32
        initq_modes_grad = bool(self._initq_modes() and self.hip_autograd_initq_modes and self.compute == "f32")
        if wants_grad and initq_modes_grad:
            if self.mode == 4 and (int(size[0]) < 2 or int(size[1]) < 2):
                raise ValueError(f"mode 4: the reflect-padded 3x3 head needs an output of at least 2 x 2, got {int(size[0])} x {int(size[1])}")
            _require_cuda(x, "x")
            from .initq_modes_training import decode_with_grad as decode_initq_modes_with_grad
            return decode_initq_modes_with_grad(self, x, size)
        if wants_grad and self._initq_modes():
            raise NotImplementedError(
                f"diinn_amd: init_q=True with mode {self.mode} (ImplicitDecoder.hip_initq_modes) is inference only: autograd "
                "through it is not covered, and hip_autograd / hip_autograd_mode4 do not open it; call it under "
                "torch.no_grad() or with bsize given")
        # reference: bsize=None runs step() under autograd (training, sr_module.py:128).  What this path cannot
        # differentiate is refused before anything looks at the tensor's device: the answer depends on no tensor data
        initq_grad = self.init_q and self.hip_autograd and self.mode == 3 and self.compute == "f32"     # the opt-in (initq_training.py)
        mode4_grad = self.mode == 4 and self.hip_autograd_mode4 and not self.init_q and self.compute == "f32"   # the opt-in (mode4_training.py)
        # the opt-in (split_training.py): mode 3, init_q=False, the split-bf16 arithmetic both ways
        split_grad = bool(self.hip_autograd_split_bf16 and self.mode == 3 and not self.init_q and self.compute == "bf16x3")
        if wants_grad and not mode4_grad and not split_grad and (self.mode not in (1, 2, 3) or self.compute != "f32" or (self.init_q and not initq_grad)):
            raise NotImplementedError(
                "diinn_amd: autograd through the HIP decode path covers modes 1-3 in fp32 with init_q=False (mode 3 is the "
                "reference's final model, modes 1/2 its ablations); call mode 4, init_q=True or the bf16 path under "
                "torch.no_grad() (mode 4 in fp32 with init_q=False trains once ImplicitDecoder.hip_autograd_mode4 is set)")
        if wants_grad and mode4_grad and (int(size[0]) < 2 or int(size[1]) < 2):
            raise ValueError(f"mode 4: the reflect-padded 3x3 head needs an output of at least 2 x 2, got {int(size[0])} x {int(size[1])}")
        initq_x3 = bool(self.init_q and self.mode == 3 and self.hip_initq_split_bf16 and self.compute == "bf16x3")   # the opt-in
        if self.init_q and self.compute != "f32" and not initq_x3:
            raise ValueError("init_q=True runs in fp32 only")
        _require_cuda(x, "x")
        if wants_grad:
            if split_grad:
                from .split_training import decode_with_grad as decode_split_with_grad
                return decode_split_with_grad(self, x, size)
            if self.init_q:
                from .initq_training import decode_with_grad as decode_initq_with_grad
                return decode_initq_with_grad(self, x, size)
            if self.mode == 4:
                from .mode4_training import decode_with_grad as decode_mode4_with_grad
                return decode_mode4_with_grad(self, x, size)
            from .training import decode_with_grad
            return decode_with_grad(self, x, size)
        b, c, h, w = x.shape
        need = b * h * w * P_CHANNELS
        capturing = torch.cuda.is_current_stream_capturing()
        key = None if capturing else (str(x.device), torch.cuda.current_stream(x.device).cuda_stream)

        def cached(cache, numel):
            # hipGraph capture (modules._GraphReplay): the captured kernels keep the workspace pointer for the
            # graph's lifetime, so it must come from the graph's private pool -- the cached workspace is
            # replaced (and its block recycled) as soon as a larger input arrives
            if capturing:
                return torch.empty(numel, dtype=torch.float32, device=x.device)
            ws = cache.get(key)
            if ws is None or ws.numel() < numel:
                cache.pop(key, None)
                while len(cache) >= self._MAX_WORKSPACES:
                    cache.pop(next(iter(cache)))
                ws = cache[key] = torch.empty(numel, dtype=torch.float32, device=x.device)
            return ws

        if self._initq_modes():
            hu, wu = size
            hu, wu = int(hu), int(wu)
            if self.mode == 4 and (hu < 2 or wu < 2):
                raise ValueError(f"mode 4: the reflect-padded 3x3 head needs an output of at least 2 x 2, got {hu} x {wu}")
            # mode 4 computes the planes and the taps of one more row each way (clipped to the image): THOSE rows follow the chunk
            # rule -- within the cap and a whole number of the kernels' 8-row blocks, as MODE4_CHUNK_ROWS = 254 does without
            # init_q -- so a chunk is two output rows shorter (16 + 2 tap rows would start a third block row of both kernels:
            # B = 16 of 48 x 48 x4 measured 22.8 ms that way against the eager sequence's 21.4)
            halo = 2 if self.mode == 4 else 0
            chunk = initq_chunk_rows(b, wu, self.INITQ_CHUNK_BYTES) - halo
            pix = cached(self._pix_workspaces, b * min(chunk + halo, hu) * wu * (P_CHANNELS + HIDDEN))
            taps = cached(self._tap_workspaces, _native.load().diinn_mode4_taps_bytes(b, hu, wu, 1, min(hu, chunk + 1)) // 4) \
                if self.mode == 4 else None
            with torch.no_grad():
                packed = self.packed_weights(x.device)
                out = torch.empty((b, 3, hu, wu), dtype=torch.float32, device=x.device)
                for y0 in range(0, hu, chunk):
                    decode_features_initq(x, packed, self._packed_initq, (hu, wu), self.mode, head=self._packed_head, taps=taps,
                                          pix=pix, rows=(y0, min(hu, y0 + chunk)), out=out, sin_mode=self.sin_mode)
                return out
        if self.init_q:
            hu, wu = size
            hu, wu = int(hu), int(wu)
            chunk = initq_chunk_rows(b, wu, self.INITQ_CHUNK_BYTES)
            pix = cached(self._pix_workspaces, b * min(chunk, hu) * wu * (P_CHANNELS + HIDDEN))
            with torch.no_grad():
                packed = self.packed_weights(x.device)
                out = torch.empty((b, 3, hu, wu), dtype=torch.float32, device=x.device)
                for y0 in range(0, hu, chunk):
                    decode_features(x, packed, (hu, wu), out=out, rows=(y0, min(hu, y0 + chunk)), sin_mode=self.sin_mode,
                                    initq=self._packed_initq, pix=pix, compute="bf16x3" if initq_x3 else "f32",
                                    initq_x3=self._packed_initq_x3 if initq_x3 else None)
                return out
        workspace = cached(self._workspaces, need)
        modes_x3 = bool(self.hip_modes_split_bf16 and self.mode in (1, 2, 4) and self.compute == "bf16x3")      # the opt-in
        with torch.no_grad():
            packed = self.packed_weights(x.device)
            if self.mode != 4:
                return decode_features(x, packed, size, workspace=workspace, sin_mode=self.sin_mode,
                                       compute=self.compute, mode=self.mode, modes_x3=modes_x3)
            if self.compute != "f32" and not modes_x3:
                raise ValueError("mode 4 runs in fp32 only")
            hu, wu = size
            hu, wu = int(hu), int(wu)
            if hu < 2 or wu < 2:
                raise ValueError(f"mode 4: the reflect-padded 3x3 head needs an output of at least 2 x 2, got {hu} x {wu}")
            chunk = self.MODE4_CHUNK_ROWS
            # (rows [0, chunk + 1) reach one tap row each way unless the image ends first: the largest band of the loop below)
            taps = cached(self._tap_workspaces, _native.load().diinn_mode4_taps_bytes(b, hu, wu, 1, min(hu, chunk + 1)) // 4)
            out = torch.empty((b, 3, hu, wu), dtype=torch.float32, device=x.device)
            for y0 in range(0, hu, chunk):
                decode_features(x, packed, (hu, wu), out=out, workspace=workspace, rows=(y0, min(hu, y0 + chunk)),
                                sin_mode=self.sin_mode, mode=4, head=self._packed_head, taps=taps,
                                compute="bf16x3" if modes_x3 else "f32", modes_x3=modes_x3)
            return out
