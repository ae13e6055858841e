"""The formula sheets of the decoder paths: what the kernels compute, restated in torch tensor algebra on any device.  Tests, tools
and the documents cite them (as ``decoder.initq_forward_reference`` ...: ``decoder.py`` re-exports the public names); nothing on
the hot path calls them.  Pure torch and numpy; the library is asked only for the axis tables and the small-output rule.

First the pieces every sheet shares -- the tensor getter, the geometry of an upsampling (index tensors, ``rel_h`` / ``rel_w`` planes,
``ratio``; as ``syn`` planes or through the kernels' one-rounding fma chain), the unfold-and-gather of ``x'``, the split-bf16
product, the sine of revolutions, the reflect-padded 27-tap head -- then the four sheets, each the algebra that is its own.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch

from . import _native

HIDDEN = 256
P_CHANNELS = 1024
UNFOLD = 576
INV_2PI_F32 = float(np.float32(0.15915494309189533577))     # fp32(1 / (2 pi)): the factor the host packers multiply by


def axis_tables(n_in: int, n_out: int, small_output: bool = False) -> Tuple[np.ndarray, np.ndarray]:
    """Host tables (idx int32, rel fp32) from the C ABI ``diinn_make_axis_tables``."""
    lib = _native.load()
    idx = np.empty(n_out, np.int32)
    rel = np.empty(n_out, np.float32)
    st = lib.diinn_make_axis_tables(n_in, n_out, int(small_output),
                                    idx.ctypes.data_as(_native._i32), _native.fptr(rel))
    _native.check(st, "diinn_make_axis_tables")
    return idx, rel


# ---------------------------------------------------------------------------
# the shared pieces
# ---------------------------------------------------------------------------
def tensor_getter(sd, prefix: str, device, dtype):
    """``get(name, shape)``: ``sd[prefix + name]`` (a tensor or an array) on ``device`` in ``dtype``, reshaped."""
    def get(name, shape):
        t = sd[prefix + name]
        t = t.detach() if isinstance(t, torch.Tensor) else torch.from_numpy(np.asarray(t))
        return t.to(device=device, dtype=dtype).reshape(shape)
    return get


class Geometry(NamedTuple):
    """An [h, w] map decoded to [hu, wu]: the LR cell (iy, ix) and the fp32 offsets (rel_h, rel_w) per HR row / column, from
    ``axis_tables`` (the reference computes them in fp32 whatever the module's dtype), and ``ratio`` = h w / (hu wu) as a double."""
    hu: int
    wu: int
    n: int
    iy: torch.Tensor
    ix: torch.Tensor
    rel_h: torch.Tensor
    rel_w: torch.Tensor
    ratio: float


def geometry(h: int, w: int, size, dev) -> Geometry:
    hu, wu = int(size[0]), int(size[1])
    small = bool(_native.load().diinn_uses_small_output_kernel(hu, wu))
    iy, rel_h = axis_tables(h, hu, small)
    ix, rel_w = axis_tables(w, wu, small)
    return Geometry(hu, wu, hu * wu, torch.from_numpy(iy.astype(np.int64)).to(dev), torch.from_numpy(ix.astype(np.int64)).to(dev),
                    torch.from_numpy(rel_h).to(dev), torch.from_numpy(rel_w).to(dev), (h * w) / (hu * wu))


def syn_planes(g: Geometry, dtype) -> torch.Tensor:
    """[3, n]: (rel_h, rel_w, ratio) per HR pixel in ``dtype``; ``ratio`` is the double rounded to it, as ``x.new_tensor`` does."""
    syn = torch.empty((3, g.hu, g.wu), dtype=dtype, device=g.iy.device)
    syn[0] = g.rel_h.to(dtype)[:, None]
    syn[1] = g.rel_w.to(dtype)[None, :]
    syn[2] = torch.tensor(g.ratio, dtype=dtype, device=g.iy.device)
    return syn.reshape(3, g.n)


def coordinate_fma(g: Geometry, wgt: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """[C, n] fp32: ``wgt`` [C,3] . (rel_h, rel_w, ratio) + ``bias`` [C,1] by the kernels' fp32 fma sequence
    ``fma(w_h, rel_h, fma(w_w, rel_w, fma(w_r, ratio, bias)))``, one rounding each (the fp32 product is exact in float64)."""
    f32, dev = torch.float32, g.iy.device

    def fma(a_, b_, c_):
        return (a_.double() * b_.double() + c_.double()).to(f32)

    relh = g.rel_h.to(f32)[:, None].expand(g.hu, g.wu).reshape(1, g.n)
    relw = g.rel_w.to(f32)[None, :].expand(g.hu, g.wu).reshape(1, g.n)
    ratio = torch.tensor(np.float32(g.ratio), dtype=f32, device=dev)
    a = fma(wgt[:, 2:3], ratio, bias)
    a = fma(wgt[:, 1:2], relw, a)
    return fma(wgt[:, 0:1], relh, a)


def gather_unfold(x: torch.Tensor, g: Geometry) -> torch.Tensor:
    """[b, c * 9, n]: X[:, iy, ix] per HR pixel, X = unfold3x3(x), index c * 9 + 3 ky + kx, zero padded."""
    b, c, h, w = x.shape
    unf = torch.nn.functional.unfold(x, 3, padding=1).view(b, c * 9, h, w)
    return unf[:, :, g.iy][:, :, :, g.ix].reshape(b, c * 9, g.n)


def split_hi_lo(v: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """hi = bf16(v), lo = bf16(v - hi), round to nearest even, both returned in v's dtype (fp32)."""
    hi = v.to(torch.bfloat16).to(v.dtype)
    lo = (v - hi).to(torch.bfloat16).to(v.dtype)
    return hi, lo


def split_matmul(w: torch.Tensor, q: torch.Tensor) -> torch.Tensor:
    """The split-bf16 product of DESIGN.md 3.5, w . q as the kernels form it: ``(w_lo . q_hi + w_hi . q_lo) + w_hi . q_hi``, the two
    small products first, the leading one last; accumulated in the operands' dtype (torch matmuls, not the MFMA's summation order)."""
    wh, wl = split_hi_lo(w)
    qh, ql = split_hi_lo(q)
    return (wl @ qh + wh @ ql) + wh @ qh


def sin_rev(a: torch.Tensor) -> torch.Tensor:
    """sin of an argument in revolutions, taken in float64 and rounded to the argument's dtype."""
    return torch.sin(a.double() * (2.0 * math.pi)).to(a.dtype)


def reflect_index(n: int, dev) -> torch.Tensor:
    """[n + 2]: the source position of padded position -1 .. n under 'reflect' (-1 -> 1, n -> n - 2)."""
    r = torch.arange(-1, n + 1, device=dev).abs()
    return torch.where(r >= n, 2 * (n - 1) - r, r)


def head3x3_gather(taps: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """The reflect-padded 9-point gather of mode 4's head (``head3x3_reflect_kernel``): ``taps`` [3 (ky), 3 (kx), d0, d1, Hu, Wu] holds
    T[ky][kx] of every pixel, ``bias`` broadcasts to [d0, d1, Hu, Wu]; out[.., y, x] = bias + sum T[ky][kx][.., refl(y + ky - 1),
    refl(x + kx - 1)], added in (ky, kx) order."""
    hu, wu = taps.shape[-2:]
    ry, rx = reflect_index(hu, taps.device), reflect_index(wu, taps.device)
    out = bias.expand(taps.shape[2:]).clone()
    for ky in range(3):
        for kx in range(3):
            out = out + taps[ky, kx][:, :, ry[ky:ky + hu]][:, :, :, rx[kx:kx + wu]]
    return out


def head3x3(get, q: torch.Tensor, g: Geometry) -> torch.Tensor:
    """Mode 4's head on q_3 [b,256,n] -> [b,3,Hu,Wu]: the 27 tap values per pixel, T[ky][kx][c] = Lw[c, :, ky, kx] . q_3, then the
    gather."""
    b = q.shape[0]
    taps = torch.einsum("chyx,bhn->byxcn", get("last_layer.weight", (3, HIDDEN, 3, 3)), q).reshape(b, 3, 3, 3, g.hu, g.wu)
    return head3x3_gather(taps.permute(1, 2, 0, 3, 4, 5), get("last_layer.bias", (1, 3, 1, 1)))


def head1x1(get, q: torch.Tensor, g: Geometry) -> torch.Tensor:
    """out = L . q_3 + bL -> [b,3,Hu,Wu]."""
    return (get("last_layer.weight", (3, HIDDEN)) @ q + get("last_layer.bias", (3, 1))).reshape(q.shape[0], 3, g.hu, g.wu)


def _stacked_k(get):
    """(Wx [1024,576], bK [1,1024,1]): the feature columns of K_0..3 and their biases, stacked as the pixel record orders them."""
    wx = torch.cat([get("K.0.0.weight", (HIDDEN, UNFOLD))] +
                   [get(f"K.{i}.0.weight", (HIDDEN, HIDDEN + UNFOLD))[:, HIDDEN:] for i in (1, 2, 3)], 0)
    return wx, torch.cat([get(f"K.{i}.0.bias", (HIDDEN,)) for i in range(4)])[None, :, None]


def _k_layers(get, mode: int):
    """([K_1, K_2, K_3], [bK_0 .. bK_3] as columns) of modes 1 (K_i [256,256]), 2 and 4 (K_i [256,832])."""
    kin = HIDDEN if mode == 1 else HIDDEN + UNFOLD
    return [get(f"K.{i}.0.weight", (HIDDEN, kin)) for i in (1, 2, 3)], [get(f"K.{i}.0.bias", (HIDDEN, 1)) for i in range(4)]


# ---------------------------------------------------------------------------
# the sheets
# ---------------------------------------------------------------------------
def initq_planes_reference(sd, feat, size, arith: str = "split", prefix: str = "") -> torch.Tensor:
    """The pixel planes of the split-bf16 ``init_q`` path, [B, Hu*Wu, 1280] (channels 1024.. in REVOLUTIONS), as
    ``initq_planes_x3_kernel`` forms them: everything that feeds a sine divided by fp32(1/(2 pi)) in fp32, ``E`` by the kernel's
    fp32 fma sequence (ratio, rel_w, rel_h) with the sine taken in float64, ``x' = E * X`` in fp32.  ``arith`` = "split": both GEMMs
    as ``split_matmul`` in fp32 (torch matmuls, not the MFMA's summation order); "f64": the float64 products of the same fp32
    operands, the yardstick of the planes test."""
    if arith not in ("split", "f64"):
        raise ValueError(f"arith must be 'split' or 'f64', got {arith!r}")
    f32 = torch.float32
    get = tensor_getter(sd, prefix, feat.device, f32)
    inv = torch.tensor(INV_2PI_F32, dtype=f32, device=feat.device)
    x = feat.to(f32)
    b, _, h, w = x.shape
    g = geometry(h, w, size, feat.device)
    e = sin_rev(coordinate_fma(g, get("first_layer.0.weight", (UNFOLD, 3)) * inv, get("first_layer.0.bias", (UNFOLD, 1)) * inv))
    xp = e[None] * gather_unfold(x, g)                        # [b, 576, n], fp32
    wx, bk = _stacked_k(get)
    q0w, q0b = get("Q.0.0.weight", (HIDDEN, UNFOLD)) * inv, get("Q.0.0.bias", (HIDDEN, 1)) * inv
    if arith == "f64":
        pk = wx.double() @ xp.double() + bk.double()
        a0 = q0w.double() @ e.double() + q0b.double()
    else:
        pk = split_matmul(wx, xp) + bk
        a0 = split_matmul(q0w, e) + q0b
    return torch.cat([pk, a0[None].expand(b, HIDDEN, g.n)], 1).transpose(1, 2).contiguous()


def _initq_forward_split(sd, feat, size, dtype, prefix: str) -> torch.Tensor:
    """``initq_forward_reference(..., split_bf16=True)``: the three split stages -- both planes GEMMs (``initq_planes_reference``),
    and the two 256 x 256 products of layers 1..3 -- with every sine taken of revolutions in float64."""
    get = tensor_getter(sd, prefix, feat.device, torch.float32)
    inv = torch.tensor(INV_2PI_F32, dtype=torch.float32, device=feat.device)
    hu, wu = int(size[0]), int(size[1])
    pix = initq_planes_reference(sd, feat, size, "split", prefix).transpose(1, 2)      # [b, 1280, n]
    q = torch.relu(pix[:, :HIDDEN]) * sin_rev(pix[:, P_CHANNELS:])
    for i in (1, 2, 3):
        k = torch.relu(split_matmul(get(f"K.{i}.0.weight", (HIDDEN, HIDDEN + UNFOLD))[:, :HIDDEN], q) + pix[:, HIDDEN * i:HIDDEN * (i + 1)])
        s = split_matmul(get(f"Q.{i}.0.weight", (HIDDEN, HIDDEN)) * inv, q) + get(f"Q.{i}.0.bias", (HIDDEN, 1)) * inv
        q = k * sin_rev(s)
    out = get("last_layer.weight", (3, HIDDEN)) @ q + get("last_layer.bias", (3, 1))
    return out.reshape(pix.shape[0], 3, hu, wu).to(dtype)


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
    get = tensor_getter(sd, prefix, feat.device, dtype)
    x = feat.to(dtype)
    b, _, h, w = x.shape
    g = geometry(h, w, size, feat.device)
    e = torch.sin(get("first_layer.0.weight", (UNFOLD, 3)) @ syn_planes(g, dtype) + get("first_layer.0.bias", (UNFOLD, 1)))   # [576, n]
    xp = e[None] * gather_unfold(x, g)                                                                             # [b, 576, n]
    wx, bk = _stacked_k(get)
    pix = wx @ xp + bk                                                                                             # [b, 1024, n]
    a0 = get("Q.0.0.weight", (HIDDEN, UNFOLD)) @ e + get("Q.0.0.bias", (HIDDEN, 1))                                # [256, n]
    q = torch.relu(pix[:, :HIDDEN]) * torch.sin(a0)[None]
    if planes is not None:
        planes.append((torch.relu(pix[:, :HIDDEN]), a0[None].expand(b, HIDDEN, g.n)))
    for i in (1, 2, 3):
        k = torch.relu(get(f"K.{i}.0.weight", (HIDDEN, HIDDEN + UNFOLD))[:, :HIDDEN] @ q + pix[:, HIDDEN * i:HIDDEN * (i + 1)])
        s = get(f"Q.{i}.0.weight", (HIDDEN, HIDDEN)) @ q + get(f"Q.{i}.0.bias", (HIDDEN, 1))
        if planes is not None:
            planes.append((k, s))
        q = k * torch.sin(s)
    return head1x1(get, q, g)


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
    get = tensor_getter(sd, prefix, feat.device, dtype)
    x = feat.to(dtype)
    g = geometry(x.shape[2], x.shape[3], size, feat.device)
    e = torch.sin(get("first_layer.0.weight", (UNFOLD, 3)) @ syn_planes(g, dtype) + get("first_layer.0.bias", (UNFOLD, 1)))   # [576, n]
    xp = e[None] * gather_unfold(x, g)                                                                               # [b, 576, n]
    kw, bk = _k_layers(get, mode)
    k = torch.relu(get("K.0.0.weight", (HIDDEN, UNFOLD)) @ xp + bk[0])                                              # PIX[0:256]
    q = k * torch.sin(get("Q.0.0.weight", (HIDDEN, UNFOLD)) @ e + get("Q.0.0.bias", (HIDDEN, 1)))[None]           # PIX[1024:1280]
    for i in (1, 2, 3):
        seed = bk[i] if mode == 1 else kw[i - 1][:, HIDDEN:] @ xp + bk[i]                                         # PIX[256 i : 256 i + 256]
        k = torch.relu(kw[i - 1][:, :HIDDEN] @ (q if mode == 4 else k) + seed)
        q = k * torch.sin(get(f"Q.{i}.0.weight", (HIDDEN, HIDDEN)) @ q + get(f"Q.{i}.0.bias", (HIDDEN, 1)))
    return head3x3(get, q, g) if mode == 4 else head1x1(get, q, g)


def modes_x3_forward_reference(sd, feat, size, mode: int, prefix: str = "") -> torch.Tensor:
    """The EMULATION sheet of the split-bf16 arithmetic of decoder modes 1, 2 and 4 with ``init_q=False``
    (``decode_features(..., compute="bf16x3", modes_x3=True)``), in fp32 torch algebra on any device; beside
    ``initq_forward_reference(..., split_bf16=True)``, which states mode 3 with ``init_q=True``.

    What is split: the three synthesis products ``Q_i . q_{i-1}``, i = 1..3, of every mode, and for mode 4 the three modulation
    products ``K_i[:, :256] . q_{i-1}`` as well.  Every operand of such a product is carried as hi = bf16(v), lo = bf16(v - hi) and
    the product formed as ``(w_lo.q_hi + w_hi.q_lo) + w_hi.q_hi`` in fp32 (``split_matmul``: torch matmuls, not the MFMA's summation
    order).  The synthesis branch runs in REVOLUTIONS: Q_0..3 and their biases are multiplied by fp32(1/(2 pi)) in fp32 before the
    split, as the body image holds them, and every sine is taken of revolutions in float64 (``sin_rev``).

    What stays fp32: the hoisted conv ``P = Wx . unfold3x3(feat) + bK`` (mode 1: ``P_i = bK_i`` for i >= 1), the per-cell
    modulation chain of modes 1/2, ``k_0 = relu(P_0)``, ``k_i = relu(K_i[:, :256] . k_{i-1} + P_i)`` (``cell_chain_kernel``), layer
    0 with the kernels' fma sequence ``a = fma(Q0_h, rel_h, fma(Q0_w, rel_w, fma(Q0_r, ratio, bQ0)))``, the seeds and biases, and
    the head on the unsplit ``q_3``: ``L . q_3 + bL`` (modes 1/2), or the 27 tap values per pixel and the reflect-padded 9-point
    gather (mode 4)."""
    if mode not in (1, 2, 4):
        raise ValueError(f"modes_x3_forward_reference states modes 1, 2 and 4, got {mode}")
    f32 = torch.float32
    get = tensor_getter(sd, prefix, feat.device, f32)
    inv = torch.tensor(INV_2PI_F32, dtype=f32, device=feat.device)
    x = feat.to(f32)
    b, _, h, w = x.shape
    g = geometry(h, w, size, feat.device)
    kw, bk = _k_layers(get, mode)
    unf = torch.nn.functional.unfold(x, 3, padding=1)                                   # [b, 576, h*w], fp32
    P = [get("K.0.0.weight", (HIDDEN, UNFOLD)) @ unf + bk[0]]
    for i in (1, 2, 3):
        P.append(bk[i].expand(b, HIDDEN, h * w) if mode == 1 else kw[i - 1][:, HIDDEN:] @ unf + bk[i])
    cell = (g.iy[:, None] * w + g.ix[None, :]).reshape(g.n)                             # LR cell of every HR pixel
    if mode != 4:                                                                       # the per-cell chain, fp32
        kc = [torch.relu(P[0])]
        for i in (1, 2, 3):
            kc.append(torch.relu(kw[i - 1][:, :HIDDEN] @ kc[-1] + P[i]))
    a = coordinate_fma(g, get("Q.0.0.weight", (HIDDEN, 3)) * inv, get("Q.0.0.bias", (HIDDEN, 1)) * inv)
    q = torch.relu(P[0][:, :, cell]) * sin_rev(a)[None]                                 # [b, 256, n]
    for i in (1, 2, 3):
        s = split_matmul(get(f"Q.{i}.0.weight", (HIDDEN, HIDDEN)) * inv, q) + get(f"Q.{i}.0.bias", (HIDDEN, 1)) * inv
        if mode == 4:
            k = torch.relu(split_matmul(kw[i - 1][:, :HIDDEN], q) + P[i][:, :, cell])
        else:
            k = kc[i][:, :, cell]
        q = k * sin_rev(s)
    return head3x3(get, q, g) if mode == 4 else head1x1(get, q, g)


def initq_modes_x3_forward_reference(sd, feat, size, mode: int, prefix: str = "") -> torch.Tensor:
    """The EMULATION sheet of the split-bf16 arithmetic of ``init_q=True`` with decoder modes 1, 2 and 4
    (``decode_features_initq(..., compute="bf16x3")``), in fp32 torch algebra on any device; beside
    ``initq_forward_reference(..., split_bf16=True)`` (mode 3) and ``modes_x3_forward_reference`` (``init_q=False``).

    What is split (``split_matmul``: every operand as hi = bf16(v), lo = bf16(v - hi), the product ``(w_lo.x_hi + w_hi.x_lo) +
    w_hi.x_hi`` in fp32 torch matmuls, not the MFMA's summation order): both planes GEMMs on ``E`` and ``x'`` as
    ``initq_planes_reference`` forms them (mode 1: ``K_0`` and ``Q_0`` only, the seeds of layers 1..3 are ``bK_i``); the
    per-pixel chain of modes 1/2, ``k_i = relu(split_matmul(K_i[:, :256], k_{i-1}) + seed_i)`` (``pixel_chain_x3_kernel``); mode
    4's ``K_i[:, :256] . q_{i-1}``; and the synthesis products on ``Q_i * fp32(1/(2 pi))``.  The synthesis branch runs in
    REVOLUTIONS and every sine is taken of revolutions in float64 (``sin_rev``).

    What stays fp32: ``E``'s fma sequence, ``x' = E * X``, seeds, biases, ReLU, and the head on the unsplit ``q_3`` -- ``L . q_3 +
    bL`` (modes 1/2) or the 27 tap values per pixel and the reflect-padded 9-point gather (mode 4)."""
    if mode not in (1, 2, 4):
        raise ValueError(f"initq_modes_x3_forward_reference states modes 1, 2 and 4 (mode 3: initq_forward_reference(split_bf16=True)), got {mode}")
    f32 = torch.float32
    get = tensor_getter(sd, prefix, feat.device, f32)
    inv = torch.tensor(INV_2PI_F32, dtype=f32, device=feat.device)
    x = feat.to(f32)
    g = geometry(x.shape[2], x.shape[3], size, feat.device)
    e = sin_rev(coordinate_fma(g, get("first_layer.0.weight", (UNFOLD, 3)) * inv, get("first_layer.0.bias", (UNFOLD, 1)) * inv))
    xp = e[None] * gather_unfold(x, g)                                                  # [b, 576, n], fp32
    kw, bk = _k_layers(get, mode)
    k = torch.relu(split_matmul(get("K.0.0.weight", (HIDDEN, UNFOLD)), xp) + bk[0])     # PIX[0:256]
    a0 = split_matmul(get("Q.0.0.weight", (HIDDEN, UNFOLD)) * inv, e) + get("Q.0.0.bias", (HIDDEN, 1)) * inv   # PIX[1024:1280]
    q = k * sin_rev(a0)[None]
    for i in (1, 2, 3):
        seed = bk[i] if mode == 1 else split_matmul(kw[i - 1][:, HIDDEN:], xp) + bk[i]  # PIX[256 i : 256 i + 256]
        k = torch.relu(split_matmul(kw[i - 1][:, :HIDDEN], q if mode == 4 else k) + seed)
        s = split_matmul(get(f"Q.{i}.0.weight", (HIDDEN, HIDDEN)) * inv, q) + get(f"Q.{i}.0.bias", (HIDDEN, 1)) * inv
        q = k * sin_rev(s)
    return head3x3(get, q, g) if mode == 4 else head1x1(get, q, g)


def liif_x3_forward_reference(sd, feat, size, prefix: str = "imnet.") -> torch.Tensor:
    """The EMULATION sheet of the split-bf16 arithmetic of the LIIF comparison decoder (``liif_decode_features(..., split=...)``,
    ``liif_x3_kernel``), in fp32 torch algebra on any device: the reference's form (liif.py:59-127) with the three hidden
    256 x 256 layers ``imnet.layers.{2,4,6}`` as ``split_matmul(W, x^T) + b`` -- every operand carried as hi = bf16(v),
    lo = bf16(v - hi), the product ``(w_lo.x_hi + w_hi.x_lo) + w_hi.x_hi`` in fp32 (torch matmuls, not the MFMA's summation order).

    What stays fp32: the index and coordinate tables (``decoder.liif_axis_tables``), layer 0 on [unfolded features of the shifted
    nearest cell ; rel_h ; rel_w ; cell_h ; cell_w] as the reference forms it (one ``linear``; the kernel hoists its 576 feature
    columns into a conv per LR cell), the biases, the head on the unsplit activation, the areas and the blend."""
    from .decoder import liif_axis_tables
    f32 = torch.float32
    feat = feat if isinstance(feat, torch.Tensor) else torch.from_numpy(np.asarray(feat))
    dev = feat.device
    get = tensor_getter(sd, prefix, dev, f32)
    x = feat.to(f32)
    b, c, h, w = x.shape
    hu, wu = int(size[0]), int(size[1])
    unf = torch.nn.functional.unfold(x, 3, padding=1).view(b, c * 9, h, w)
    w0, b0 = get("layers.0.weight", (HIDDEN, c * 9 + 4)), get("layers.0.bias", (HIDDEN,))
    preds, areas = [], []
    for vh in (-1, 1):                                            # member order: vx outer, vy inner (liif.py:88-89)
        ih, rh, cell_h = liif_axis_tables(h, hu, vh)
        for vw in (-1, 1):
            iw, rw, cell_w = liif_axis_tables(w, wu, vw)
            q = unf[:, :, torch.from_numpy(ih.astype(np.int64)).to(dev)][:, :, :, torch.from_numpy(iw.astype(np.int64)).to(dev)]
            rel = torch.empty((b, hu, wu, 4), dtype=f32, device=dev)
            rel[..., 0] = torch.from_numpy(rh).to(dev)[None, :, None]
            rel[..., 1] = torch.from_numpy(rw).to(dev)[None, None, :]
            rel[..., 2] = cell_h
            rel[..., 3] = cell_w
            z = torch.cat([q.permute(0, 2, 3, 1), rel], dim=-1).reshape(-1, c * 9 + 4)
            z = torch.relu(torch.nn.functional.linear(z, w0, b0)).t()                    # [256, b * n]
            for i in (2, 4, 6):
                z = torch.relu(split_matmul(get(f"layers.{i}.weight", (HIDDEN, HIDDEN)), z) + get(f"layers.{i}.bias", (HIDDEN, 1)))
            z = torch.nn.functional.linear(z.t(), get("layers.8.weight", (3, HIDDEN)), get("layers.8.bias", (3,)))
            preds.append(z.view(b, hu, wu, 3))
            areas.append((rel[..., 0] * rel[..., 1]).abs() + 1e-9)
    tot = torch.stack(areas).sum(dim=0)
    out = 0
    for pred, area in zip(preds, (areas[3], areas[2], areas[1], areas[0])):              # diagonal swap, liif.py:121-123
        out = out + pred * (area / tot).unsqueeze(-1)
    return out.permute(0, 3, 1, 2).contiguous()
