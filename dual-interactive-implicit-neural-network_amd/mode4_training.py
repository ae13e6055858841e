"""Training path of decoder mode 4: autograd through the HIP kernels.  Opt-in: ``ImplicitDecoder.hip_autograd_mode4``.

The reference trains by ``ImplicitDecoder.forward(x, size, None)`` under autograd (sr_module.py:127-129 -> diinn.py:170-171); mode 4
is mode 3 up to the last activation q_3 = k_3 sin(s_3), followed by ``last_layer = Conv2d(256, 3, 3, padding=1,
padding_mode='reflect')`` over the HR grid (diinn.py:89-90,140-147).  With k = 3 ky + kx, r = 3 k + c, refl(-1, n) = 1,
refl(n, n) = n - 2 and H the head image's [27][256] rows (include/diinn_hip.h "decoder mode 4")::

    T[pix, k, c]  = sum_ch Lw[c, ch, ky, kx] q_3[pix, ch]
    out[b,c,y,x]  = Lb[c] + sum_k T[b, refl(y+ky-1, Hu), refl(x+kx-1, Wu), k, c]
    dT[b,y',x',k,c] = sum of g[b,c,y,x] over the (y, x) with refl(y+ky-1, Hu) = y' and refl(x+kx-1, Wu) = x'     (g = d loss / d out)
    g_q,3[pix, ch]  = sum_r H[r][ch] dT[pix, r]
    dLw[c,ch,ky,kx] = sum_pix q_3[pix, ch] dT[pix, k, c]          dLb[c] = sum of g[:, c]

and everything below g_q,3 is mode 3's backward pass.

  forward   diinn_precompute_P_wpu, diinn_decode_train_fwd (mode 3's training forward on the BODY image, whose 1x1 head is zero: its
            ``out`` is discarded, its saved planes k_i, s_i are the point), then diinn_head3x3_from_planes:
            head3x3_taps_from_planes_kernel forms q_3 from group 3 of the planes and writes the 27 tap values per pixel,
            head3x3_reflect_kernel (the inference path's gather, unchanged) adds nine of them per output.
  backward  ``training.backward_fused`` with the head image: diinn_backward_data_head3x3 (bwd_head3x3_kernel: dT, g_q,3 and layer
            3's gates; then bwd_layer_kernel for layers 3, 2, 1), dLw as seven diinn_plane_rowdot products of q_3 against the dT
            groups; the rest is mode 3's code.  ``backward_from_saved_mode4`` states the same gradients in device-agnostic tensor
            algebra, next to ``forward_torch_mode4``, a differentiable restatement of the forward: the unit-tested formula sheet (CPU,
            against the reference's own .grad fixtures) and the on-GPU cross-check of the kernels.

Two weight images travel with a step, both rebuilt on the device after an optimiser step: the body image (mode 3's training image of
the 16 K / Q tensors with a zero 1x1 head) and the head image (``pack_head3x3_on_device``, bit-equal to ``diinn_pack_head3x3``).
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F

from . import _native
from .decoder import require_2x2
from .training import (HIDDEN, PARAM_NAMES, backward_from_saved, backward_fused, checked_features, coordinate_tensors,
                       function_grads, kept, named_params, pack_on_device, param_shapes, train_forward_mode3, weights_key)

TAPS = 27                  # 9 taps x 3 colours per HR pixel
TAP_STRIDE = 28            # floats per pixel of the tap buffer (one pad float)
MODE4_PARAM_SHAPES: Dict[str, Tuple[int, ...]] = param_shapes(4)


def pack_head3x3_on_device(lw: torch.Tensor, lb: torch.Tensor) -> torch.Tensor:
    """``decoder.pack_head3x3`` of ``last_layer.weight`` [3,256,3,3] / ``last_layer.bias`` [3] on their own device (CPU tensors too),
    bit-equal to the C ABI's ``diinn_pack_head3x3``: rows [27][256] with row 3 (3 ky + kx) + c = Lw[c, :, ky, kx], then Lb, then the
    validity word DIINN_HEAD3X3_MAGIC.  A permutation and a fill: no host synchronisation."""
    if tuple(lw.shape) != (3, HIDDEN, 3, 3) or tuple(lb.shape) != (3,):
        raise ValueError(f"expected last_layer.weight [3,{HIDDEN},3,3] and last_layer.bias [3], got {tuple(lw.shape)} and {tuple(lb.shape)}")
    rows = lw.detach().to(torch.float32).permute(2, 3, 0, 1).reshape(TAPS * HIDDEN)
    image = torch.cat([rows, lb.detach().to(torch.float32).reshape(3), rows.new_zeros(1)])
    image[TAPS * HIDDEN + 3:].view(torch.int32).fill_(_native.HEAD3X3_MAGIC)
    return image


_zero_heads: Dict[str, Tuple[torch.Tensor, torch.Tensor]] = {}


def images_on_device(params: Sequence[torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
    """(body image, head image) of the PARAM_NAMES tensors of a mode-4 decoder on their GPU.  The body image is
    ``training.pack_on_device`` over the 16 K / Q tensors with a zero 1x1 head (layout 3; the zeros are kept per device, so the
    image's cache key is stable); both are kept while no parameter has been modified."""
    dev = params[0].device
    zeros = _zero_heads.get(str(dev))
    if zeros is None:
        zeros = _zero_heads[str(dev)] = (torch.zeros((3, HIDDEN, 1, 1), device=dev), torch.zeros(3, device=dev))
    body = pack_on_device([*params[:16], *zeros], 4)
    lw, lb = params[16], params[17]
    return body, kept("head4", (str(dev), *weights_key((lw, lb))), (lw, lb), lambda: pack_head3x3_on_device(lw, lb))


# ---------------------------------------------------------------------------
# the formula sheet (device-agnostic tensor algebra)
# ---------------------------------------------------------------------------
def forward_torch_mode4(feat: torch.Tensor, params: Sequence[torch.Tensor], size: Sequence[int]):
    """The mode-4 forward restated in torch, differentiable, in the reference's own form and operation order (unfold, nearest-exact
    replication through the index tables, the 1x1 convolutions of step() on cat([q; x]), the reflect-padded 3x3 head; diinn.py:
    132-147,161-171) and in ``feat``'s dtype.  ``params`` in PARAM_NAMES order with mode 4's shapes.
    Returns (out [B,3,Hu,Wu], acts [4,2,256,N]: the planes k_i, s_i the training forward saves, pixel index (b*Hu + y)*Wu + x)."""
    dt, dev = feat.dtype, feat.device
    p = {name: t.to(dt) for name, t in zip(PARAM_NAMES, params)}
    b, c, h, w = feat.shape
    hu, wu = int(size[0]), int(size[1])
    n = b * hu * wu
    idx_h, rel_h, idx_w, rel_w, ratio = coordinate_tensors(h, w, hu, wu, dev)
    syn = torch.empty((b, 3, hu, wu), dtype=dt, device=dev)
    syn[:, 0] = rel_h.to(dt)[None, :, None]
    syn[:, 1] = rel_w.to(dt)[None, None, :]
    syn[:, 2] = ratio
    x = F.unfold(feat, 3, padding=1).view(b, c * 9, h, w)[:, :, idx_h][:, :, :, idx_w]

    def plane(t):
        return t.permute(1, 0, 2, 3).reshape(HIDDEN, n)

    acts = []
    k = torch.relu(F.conv2d(x, p["K.0.0.weight"], p["K.0.0.bias"]))
    s = F.conv2d(syn, p["Q.0.0.weight"], p["Q.0.0.bias"])
    acts.append(torch.stack([plane(k), plane(s)]))
    q = k * torch.sin(s)
    for i in (1, 2, 3):
        k = torch.relu(F.conv2d(torch.cat([q, x], dim=1), p[f"K.{i}.0.weight"], p[f"K.{i}.0.bias"]))
        s = F.conv2d(q, p[f"Q.{i}.0.weight"], p[f"Q.{i}.0.bias"])
        acts.append(torch.stack([plane(k), plane(s)]))
        q = k * torch.sin(s)
    out = F.conv2d(F.pad(q, (1, 1, 1, 1), mode="reflect"), p["last_layer.weight"], p["last_layer.bias"])
    return out, torch.stack(acts)


def _axis_sources(n: int, dev) -> Tuple[torch.Tensor, torch.Tensor]:
    """Per axis of length ``n`` and tap t = 0..2: the up to two source positions p with refl(p + t - 1, n) = p' for every p' --
    (index [3, 2, n] int64, mask [3, 2, n]): slot 0 the direct neighbour p' - t + 1 where it lies inside, slot 1 the reflected
    border (position 0 into p' = 1 for t = 0, position n - 1 into p' = n - 2 for t = 2).  The two never coincide."""
    pos = torch.arange(n, device=dev)
    idx = torch.zeros((3, 2, n), dtype=torch.int64, device=dev)
    ok = torch.zeros((3, 2, n), dtype=torch.bool, device=dev)
    for t in range(3):
        d = pos - t + 1
        ok[t, 0] = (d >= 0) & (d < n)
        idx[t, 0] = d.clamp(0, n - 1)
    ok[0, 1] = pos == 1
    ok[2, 1] = pos == n - 2
    idx[2, 1] = n - 1
    return idx, ok


def head_adjoint_taps(gout: torch.Tensor) -> torch.Tensor:
    """dT [B, 27, Hu, Wu] (row r = 3 (3 ky + kx) + c) of g = ``gout`` [B,3,Hu,Wu]: the adjoint of the reflect-padded 9-point gather,
    dT[b, r, y', x'] = sum of g[b, c, y, x] over the (y, x) with refl(y + ky - 1, Hu) = y' and refl(x + kx - 1, Wu) = x', the up to
    four terms added in bwd_head3x3_kernel's order: (direct y, direct x), (direct y, border x), (border y, direct x), (border, border)."""
    b, _, hu, wu = gout.shape
    require_2x2(hu, wu)
    iy, oy = _axis_sources(hu, gout.device)
    ix, ox = _axis_sources(wu, gout.device)
    taps = []
    for ky in range(3):
        for kx in range(3):
            acc = gout.new_zeros((b, 3, hu, wu))
            for sy in range(2):
                for sx in range(2):
                    term = gout[:, :, iy[ky, sy]][:, :, :, ix[kx, sx]]
                    acc = acc + term * (oy[ky, sy][:, None] & ox[kx, sx][None, :]).to(gout.dtype)
            taps.append(acc)
    return torch.stack(taps, dim=1).reshape(b, TAPS, hu, wu)


def backward_from_saved_mode4(gout: torch.Tensor, feat: torch.Tensor, acts: torch.Tensor, params: Sequence[torch.Tensor],
                              size: Sequence[int], need_feat_grad: bool = True
                              ) -> Tuple[Optional[torch.Tensor], List[torch.Tensor]]:
    """Gradients of the mode-4 decoder given d(loss)/d(out): the formula sheet (any device, the dtype of ``acts``).

    gout [B,3,Hu,Wu]; feat [B,64,H,W]; acts [4,2,256,N] plain planes k_i, s_i; params in PARAM_NAMES order with mode 4's shapes.
    Returns (d feat or None, [d param ...] in PARAM_NAMES order).  The head (module docstring): dT = ``head_adjoint_taps(gout)``,
    g_q,3 = H^T dT, dLw = q_3 dT^T, dLb = sum of g; below it ``training.backward_from_saved``, mode 3's formulas, unchanged."""
    dt = acts.dtype
    b, _, hu, wu = gout.shape
    n = b * hu * wu
    lw = params[PARAM_NAMES.index("last_layer.weight")].to(dt)
    hrows = lw.permute(2, 3, 0, 1).reshape(TAPS, HIDDEN)                              # H[r = 3 k + c][ch]
    d_t = head_adjoint_taps(gout.to(dt)).permute(1, 0, 2, 3).reshape(TAPS, n)         # [27, N]
    q3 = acts[3, 0] * torch.sin(acts[3, 1])
    d_lw = (d_t @ q3.t()).reshape(3, 3, 3, HIDDEN).permute(2, 3, 0, 1)                # [ky, kx, c, ch] -> [c, ch, ky, kx]
    d_lb = gout.to(dt).sum((0, 2, 3))
    g_q3 = hrows.t() @ d_t                                                            # [256, N]
    return backward_from_saved(gout, feat, acts, params, size, need_feat_grad, head=(g_q3, d_lw, d_lb))


# ---------------------------------------------------------------------------
# the HIP path
# ---------------------------------------------------------------------------
def train_forward_mode4(feat_c: torch.Tensor, params: Sequence[torch.Tensor], hu: int, wu: int, sin_mode: int):
    """The mode-4 training forward on a contiguous fp32 CUDA ``feat_c``: mode 3's on the body image (whose 1x1 head is zero: its
    ``out`` is discarded), then diinn_head3x3_from_planes.  Returns (out, acts [4,T,512,32], body image, head image)."""
    b = feat_c.shape[0]
    packed, head = images_on_device(params)
    _, acts = train_forward_mode3(feat_c, packed, hu, wu, sin_mode)
    taps = torch.empty(b * hu * wu * TAP_STRIDE, dtype=torch.float32, device=feat_c.device)
    out = torch.empty((b, 3, hu, wu), dtype=torch.float32, device=feat_c.device)
    with _native.launcher(feat_c.device) as run:
        run("diinn_head3x3_from_planes", acts, packed, head, taps, out, b, hu, wu)
    return out, acts, packed, head


class DecodeMode4Function(torch.autograd.Function):
    """out = decoder(feat) for decoder mode 4 on the HIP kernels, differentiable in feat and the 18 parameter tensors (PARAM_NAMES
    order, ``last_layer.weight`` [3,256,3,3]).  The tap buffer (112 bytes per HR pixel) is dropped after the forward; the backward
    needs the saved k_i / s_i planes, the features and the two images."""

    @staticmethod
    def forward(ctx, feat: torch.Tensor, hu: int, wu: int, sin_mode: int, *params: torch.Tensor) -> torch.Tensor:
        require_2x2(hu, wu)
        feat_c = checked_features(feat, params, PARAM_NAMES, MODE4_PARAM_SHAPES, hu, wu, 2 * HIDDEN, " for decoder mode 4")
        out, acts, packed, head = train_forward_mode4(feat_c, params, hu, wu, sin_mode)
        ctx.save_for_backward(feat_c, acts, packed, head, *[p_.detach() for p_ in params])
        ctx.size = (hu, wu)
        return out

    @staticmethod
    def backward(ctx, gout: torch.Tensor):
        feat, acts, packed, head, *params = ctx.saved_tensors
        d_feat, d_params = backward_fused(gout.contiguous(), feat, acts, params, packed, ctx.size,
                                          need_feat_grad=ctx.needs_input_grad[0], head=head)
        return function_grads(ctx, d_feat, d_params, 4)


def decode_with_grad(decoder, feat: torch.Tensor, size: Sequence[int]) -> torch.Tensor:
    """``ImplicitDecoder(mode=4, hip_autograd_mode4=True).forward(x, size, None)`` under autograd."""
    hu, wu = size
    return DecodeMode4Function.apply(feat, int(hu), int(wu), int(decoder.sin_mode), *named_params(decoder, PARAM_NAMES))
