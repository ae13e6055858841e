"""Training path of the decoder with ``init_q=True`` and modes 1, 2 and 4: autograd through the HIP kernels.
Opt-in: ``ImplicitDecoder.hip_autograd_initq_modes`` together with ``hip_initq_modes``.

The reference trains every ``ImplicitDecoder(mode, init_q)`` by ``forward(x, size, None)`` under autograd (sr_module.py:127-129 ->
diinn.py:170-171 -> step(), :113-147).  Per HR pixel E, x' = E * X[cell] and s_0 = Q0 E + bQ0 are those of mode 3 with ``init_q``
(initq_training.py); with Kk_i = K.i.weight[:, :256] and, in modes 2 and 4, Wx_i = K.i.weight[:, 256:]::

    modes 1/2   k_0 = relu(Wx_0 x' + bK_0)     k_i = relu(Kk_i k_{i-1} + seed_i)     seed_i = Wx_i x' + bK_i (mode 2), bK_i (mode 1)
                s_i = Qw_i q_{i-1} + bQ_i      q_i = k_i sin(s_i)                     out = L q_3 + bL
    mode 4      mode 3 with init_q up to q_3, then last_layer = Conv2d(256, 3, 3, padding=1, 'reflect') over the HR grid

  forward   modes 1/2: ``diinn_decode_initq_train_fwd_qonly`` -- the radians planes of the whole image, pixel_chain_kernel, then
            decode_kernel<SIN | DECODE_INITQ, KPART = false, SAVE>: k_i as the chain left it in the pixel record, s_i in radians.
            mode 4: ``diinn_decode_initq_train_fwd`` on the body image with a zero 1x1 head (its ``out`` is discarded), then
            ``diinn_head3x3_from_planes``.
  backward  ``initq_training.backward_fused_initq`` with another chain in front (its ``qonly`` / ``head``):
            modes 1/2: ``diinn_backward_data_qonly`` leaves g^_a,i = g_q,i sin(s_i) [k_i > 0] in rows 0..255 of G_i and g_s,i below; NEW:
            pixel_chain_bwd_kernel (``diinn_pixel_chain_bwd``) runs the modulation chain backwards per HR pixel,
                g_a,3 = g^_a,3      g_a,i-1 = [k_{i-1} > 0] (Kk_i^T g_a,i) + g^_a,i-1      (i = 3, 2, 1)
            in place; dKk_i = g_a,i k_{i-1}^T takes the saved k planes as its right-hand side.  mode 4: ``diinn_backward_data_head3x3``.
            Everything behind the chain -- initq_bwd_kernel, the plane GEMMs and rowdots, the cell sums and the fold -- is mode 3's.
            ``backward_from_saved_initq_modes`` states the same gradients in device-agnostic tensor algebra, next to
            ``forward_planes_initq_modes``, a restatement of the forward that returns the saved planes: the unit-tested formula sheet
            (CPU, against the reference's own .grad fixtures) and the on-GPU cross-check of the fused path.

Mode 1 (K.1..3 are [256,256]) runs mode 2's path: both images are built from K.1..3 widened with zero feature columns, so the
slots of the pixel record hold bK_i exactly, dx' gets nothing from layers 1..3 and the feature columns of dK.1..3 are dropped.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import _native
from .decoder import require_2x2
from .initq_training import (INITQ_PARAM_NAMES, INITQ_PARAM_SHAPES, PAD_ROWS, backward_fused_initq, embedding_planes,
                             pack_body_on_device, pack_train_image_on_device)
from .sheets import head3x3_gather
from .mode4_training import TAP_STRIDE, TAPS, head_adjoint_taps, pack_head3x3_on_device
from .training import (HIDDEN, PARAM_NAMES, UNFOLD, _cell_sum, _fill_wpu, checked_features, coordinate_tensors, function_grads, kept,
                       named_params, train_buffers, weights_key)

MODES = (1, 2, 4)
_K123 = tuple(f"K.{i}.0.weight" for i in (1, 2, 3))


def param_shapes(mode: int) -> Dict[str, Tuple[int, ...]]:
    """INITQ_PARAM_SHAPES for decoder ``mode`` with ``init_q``: mode 2 has mode 3's; mode 1's K.1..3 are [256,256,1,1]
    (diinn.py:53-60); mode 4's ``last_layer.weight`` is [3,256,3,3] (diinn.py:89-90)."""
    if mode not in MODES:
        raise ValueError(f"init_q training of modes 1, 2 and 4 (mode 3: initq_training.py), got mode {mode}")
    if mode == 1:
        return {**INITQ_PARAM_SHAPES, **{name: (HIDDEN, HIDDEN, 1, 1) for name in _K123}}
    if mode == 4:
        return {**INITQ_PARAM_SHAPES, "last_layer.weight": (3, HIDDEN, 3, 3)}
    return INITQ_PARAM_SHAPES


def widen_mode1(p: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """Mode 1's named tensors with K.1..3 widened to mode 2's [256,832,1,1] by zero feature columns (what ``pack_state_dict`` does on
    the host for the inference image)."""
    wide = dict(p)
    for name in _K123:
        k = p[name].detach().reshape(HIDDEN, HIDDEN)
        wide[name] = torch.cat([k, k.new_zeros((HIDDEN, UNFOLD))], 1).reshape(HIDDEN, HIDDEN + UNFOLD, 1, 1)
    return wide


def image_tensors(params: Sequence[torch.Tensor], mode: int) -> Dict[str, torch.Tensor]:
    """The named tensors the two images of a step are gathered from (mode 3's shapes): mode 1 widened, mode 4 with a zero 1x1 head."""
    p = {name: t.detach() for name, t in zip(INITQ_PARAM_NAMES, params)}
    if mode == 1:
        p = widen_mode1(p)
    if mode == 4:
        p["last_layer.weight"] = p["last_layer.weight"].new_zeros((3, HIDDEN, 1, 1))
        p["last_layer.bias"] = p["last_layer.bias"].new_zeros(3)
    return p


def images_on_device(params: Sequence[torch.Tensor], mode: int):
    """(body image, init_q training image, head image or None) of the INITQ_PARAM_NAMES tensors of a mode-``mode`` decoder on their GPU,
    each one gather (``initq_training.pack_body_on_device`` / ``pack_train_image_on_device``, ``mode4_training.pack_head3x3_on_device``).
    Mode 4's body image also carries section WPU and its validity word (``training._fill_wpu``): diinn_head3x3_from_planes answers NaN
    on a body image without one.  The last triple is kept while no parameter has been modified; the entry pins its tensors."""
    def build():
        p = image_tensors(params, mode)
        body = pack_body_on_device(p)
        head = None
        if mode == 4:
            _fill_wpu(body, [p[name] for name in PARAM_NAMES], 3)
            named = dict(zip(INITQ_PARAM_NAMES, params))
            head = pack_head3x3_on_device(named["last_layer.weight"], named["last_layer.bias"])
        return body, pack_train_image_on_device(p), head
    return kept("initq_modes", (mode, *weights_key(params)), params, build)


# ---------------------------------------------------------------------------
# the formula sheet (device-agnostic tensor algebra)
# ---------------------------------------------------------------------------
def forward_planes_initq_modes(feat: torch.Tensor, params: Sequence[torch.Tensor], size: Sequence[int], mode: int):
    """The forward of ``init_q=True`` with mode 1, 2 or 4 in tensor algebra (any device, ``feat``'s dtype), in the restructured form of
    ``decoder.initq_modes_forward_reference``.  ``params`` in INITQ_PARAM_NAMES order with ``param_shapes(mode)``.
    Returns (out [B,3,Hu,Wu], acts [4,2,256,N]: the planes k_i, s_i the training forward saves, pixel index (b*Hu + y)*Wu + x)."""
    shapes = param_shapes(mode)
    dt, dev = feat.dtype, feat.device
    p = {name: t.to(dt) for name, t in zip(INITQ_PARAM_NAMES, params)}
    for name in INITQ_PARAM_NAMES:
        if tuple(p[name].shape) != shapes[name]:
            raise ValueError(f"{name}: expected shape {shapes[name]} for decoder mode {mode} with init_q, got {tuple(p[name].shape)}")
    b = feat.shape[0]
    hu, wu = int(size[0]), int(size[1])
    n = b * hu * wu
    a, xc, _ = embedding_planes(feat, p, size)
    e = torch.sin(a).repeat(1, b)                                  # [576, N]
    xp = e * xc
    kw = [p[f"K.{i}.0.weight"].reshape(HIDDEN, -1) for i in range(4)]
    bk = [p[f"K.{i}.0.bias"].reshape(HIDDEN, 1) for i in range(4)]
    k = torch.relu(kw[0] @ xp + bk[0])
    s = p["Q.0.0.weight"].reshape(HIDDEN, UNFOLD) @ e + p["Q.0.0.bias"].reshape(HIDDEN, 1)
    acts = [torch.stack([k, s])]
    q = k * torch.sin(s)
    for i in (1, 2, 3):
        seed = bk[i] if mode == 1 else kw[i][:, HIDDEN:] @ xp + bk[i]
        k = torch.relu(kw[i][:, :HIDDEN] @ (q if mode == 4 else k) + seed)
        s = p[f"Q.{i}.0.weight"].reshape(HIDDEN, HIDDEN) @ q + p[f"Q.{i}.0.bias"].reshape(HIDDEN, 1)
        acts.append(torch.stack([k, s]))
        q = k * torch.sin(s)
    if mode != 4:
        out = p["last_layer.weight"].reshape(3, HIDDEN) @ q + p["last_layer.bias"].reshape(3, 1)
        return out.reshape(3, b, hu, wu).permute(1, 0, 2, 3).contiguous(), torch.stack(acts)
    require_2x2(hu, wu)
    taps = torch.einsum("chyx,hn->yxcn", p["last_layer.weight"], q).reshape(3, 3, 3, b, hu, wu)       # T[ky][kx][c] per pixel
    out = head3x3_gather(taps, p["last_layer.bias"].reshape(3, 1, 1, 1))
    return out.permute(1, 0, 2, 3).contiguous(), torch.stack(acts)


def backward_from_saved_initq_modes(gout: torch.Tensor, feat: torch.Tensor, acts: torch.Tensor, params: Sequence[torch.Tensor],
                                    size: Sequence[int], mode: int, need_feat_grad: bool = True
                                    ) -> Tuple[Optional[torch.Tensor], List[torch.Tensor]]:
    """Gradients of the ``init_q=True`` decoder of mode 1, 2 or 4 given d(loss)/d(out): the formula sheet (any device, the dtype of
    ``acts``), as ``initq_training.backward_from_saved_initq`` is for mode 3.

    gout [B,3,Hu,Wu]; feat [B,64,H,W]; acts [4,2,256,N] plain planes k_i, s_i (radians); params in INITQ_PARAM_NAMES order with
    ``param_shapes(mode)``.  Returns (d feat or None, [d param ...] in INITQ_PARAM_NAMES order, in those shapes).  Per HR pixel, i = 3..0,
        g^_a,i = g_q,i sin(s_i) [k_i > 0]        g_s,i = g_q,i k_i cos(s_i)
    modes 1/2:  g_q,i-1 = Qw_i^T g_s,i           g_a,3 = g^_a,3     g_a,i-1 = [k_{i-1} > 0] (Kk_i^T g_a,i) + g^_a,i-1     dKk_i = g_a,i k_{i-1}^T
    mode 4:     g_q,i-1 = Kk_i^T g_a,i + Qw_i^T g_s,i        g_a,i = g^_a,i        dKk_i = g_a,i q_{i-1}^T;   g_q,3 = H^T dT (mode4_training.py)
    and, with the completed g_a,i, everything of ``backward_from_saved_initq``:
        dx' = sum_i Wx_i^T g_a,i (mode 1: Wx_0 alone)     dWx_i = g_a,i x'^T     dbK_i = rowsum g_a,i     dQw_i = g_s,i q_{i-1}^T
        dE = dx' * X + Q0^T g_s,0     da = dE cos(a)     dQ0 = g_s,0 E^T     dFw = da syn^T     dfeat = fold3x3(per-cell sums of dx' * E)."""
    shapes = param_shapes(mode)
    dt = acts.dtype
    p = {name: t.to(dt) for name, t in zip(INITQ_PARAM_NAMES, params)}
    feat = feat.to(dt)
    b, _, h, w = feat.shape
    hu, wu = int(size[0]), int(size[1])
    n = b * hu * wu
    dev = gout.device
    idx_h, _, idx_w, _, _ = coordinate_tensors(h, w, hu, wu, dev)
    a, xc, syn = embedding_planes(feat, p, size)
    e = torch.sin(a).repeat(1, b)
    cos_a = torch.cos(a).repeat(1, b)
    syn_n = syn.repeat(1, b)
    xp = e * xc
    grads: Dict[str, torch.Tensor] = {}

    qs = [acts[i, 0] * torch.sin(acts[i, 1]) for i in range(4)]
    if mode == 4:
        d_t = head_adjoint_taps(gout.to(dt)).permute(1, 0, 2, 3).reshape(TAPS, n)         # [27, N], row r = 3 (3 ky + kx) + c
        hrows = p["last_layer.weight"].permute(2, 3, 0, 1).reshape(TAPS, HIDDEN)
        grads["last_layer.weight"] = (d_t @ qs[3].t()).reshape(3, 3, 3, HIDDEN).permute(2, 3, 0, 1)
        grads["last_layer.bias"] = gout.to(dt).sum((0, 2, 3))
        g_q = hrows.t() @ d_t
    else:
        g_out = gout.to(dt).permute(1, 0, 2, 3).reshape(3, n)
        grads["last_layer.weight"] = (g_out @ qs[3].t()).reshape(3, HIDDEN, 1, 1)
        grads["last_layer.bias"] = g_out.sum(1)
        g_q = p["last_layer.weight"].reshape(3, HIDDEN).t() @ g_out
    kk = [None] + [p[f"K.{i}.0.weight"].reshape(HIDDEN, -1)[:, :HIDDEN] for i in (1, 2, 3)]
    g_a: List[Optional[torch.Tensor]] = [None] * 4
    g_s: List[Optional[torch.Tensor]] = [None] * 4
    for i in (3, 2, 1, 0):
        k, s = acts[i, 0], acts[i, 1]
        g_a[i] = g_q * torch.sin(s) * (k > 0)
        g_s[i] = g_q * k * torch.cos(s)
        if i:
            g_q = p[f"Q.{i}.0.weight"].reshape(HIDDEN, HIDDEN).t() @ g_s[i]
            if mode == 4:
                g_q = kk[i].t() @ g_a[i] + g_q
    if mode != 4:                                                  # the modulation chain backwards, per HR pixel
        for i in (3, 2, 1):
            g_a[i - 1] = (acts[i - 1, 0] > 0) * (kk[i].t() @ g_a[i]) + g_a[i - 1]
    dxp = torch.zeros_like(xp)
    for i in range(4):
        wfull = p[f"K.{i}.0.weight"].reshape(HIDDEN, -1)
        grads[f"K.{i}.0.bias"] = g_a[i].sum(1)
        grads[f"Q.{i}.0.bias"] = g_s[i].sum(1)
        has_wx = i == 0 or mode != 1
        if has_wx:
            dxp += (wfull[:, HIDDEN:] if i else wfull).t() @ g_a[i]
        if i:
            prev = qs[i - 1] if mode == 4 else acts[i - 1, 0]
            d_kk = g_a[i] @ prev.t()
            grads[f"K.{i}.0.weight"] = (torch.cat([d_kk, g_a[i] @ xp.t()], 1) if has_wx else d_kk).reshape(shapes[f"K.{i}.0.weight"])
            grads[f"Q.{i}.0.weight"] = (g_s[i] @ qs[i - 1].t()).reshape(HIDDEN, HIDDEN, 1, 1)
        else:
            grads["K.0.0.weight"] = (g_a[0] @ xp.t()).reshape(HIDDEN, UNFOLD, 1, 1)
            grads["Q.0.0.weight"] = (g_s[0] @ e.t()).reshape(HIDDEN, UNFOLD, 1, 1)
    d_e = dxp * xc + p["Q.0.0.weight"].reshape(HIDDEN, UNFOLD).t() @ g_s[0]
    d_a = d_e * cos_a
    grads["first_layer.0.weight"] = (d_a @ syn_n.t()).reshape(UNFOLD, 3, 1, 1)
    grads["first_layer.0.bias"] = d_a.sum(1)
    d_feat = None
    if need_feat_grad:
        d_unf = _cell_sum(dxp * e, b, hu, wu, h, w, idx_h, idx_w)                      # [B, 576, H, W]
        d_feat = torch.nn.functional.fold(d_unf.reshape(b, UNFOLD, h * w), (h, w), 3, padding=1)
    return d_feat, [grads[name] for name in INITQ_PARAM_NAMES]


# ---------------------------------------------------------------------------
# the HIP path
# ---------------------------------------------------------------------------
def backward_fused_initq_modes(gout: torch.Tensor, feat: torch.Tensor, acts: torch.Tensor, packed: torch.Tensor, image: torch.Tensor,
                               size: Sequence[int], mode: int, head: Optional[torch.Tensor] = None, need_feat_grad: bool = True
                               ) -> Tuple[Optional[torch.Tensor], List[torch.Tensor]]:
    """The same gradients as ``backward_from_saved_initq_modes``, on the HIP kernels throughout: ``initq_training.backward_fused_initq``
    behind diinn_backward_data_qonly + diinn_pixel_chain_bwd (modes 1/2) or diinn_backward_data_head3x3 (mode 4, ``head`` its head
    image).  ``acts`` is the tiled buffer [4, T, 512, 32] of the training forward, ``packed`` / ``image`` the two images it ran on.
    Mode 1: the feature columns of dK.1..3 (products with the zero columns the images were widened by) are dropped."""
    if mode not in MODES:
        raise ValueError(f"backward_fused_initq_modes covers decoder modes 1, 2 and 4, got {mode}")
    if (mode == 4) != (head is not None):
        raise ValueError("mode 4 takes its head image, modes 1 and 2 take none")
    d_feat, d_params = backward_fused_initq(gout, feat, acts, packed, image, size, need_feat_grad=need_feat_grad,
                                            qonly=mode != 4, head=head)
    if mode == 1:
        d_params = [g.reshape(HIDDEN, HIDDEN + UNFOLD)[:, :HIDDEN].reshape(HIDDEN, HIDDEN, 1, 1) if name in _K123 else g
                    for name, g in zip(INITQ_PARAM_NAMES, d_params)]
    return d_feat, d_params


def train_forward_initq_modes(feat_c: torch.Tensor, params: Sequence[torch.Tensor], hu: int, wu: int, sin_mode: int, mode: int):
    """The training forward on a contiguous fp32 CUDA ``feat_c``.  Returns (out, acts [4,T,512,32], body image, training image, head
    image or None).  The pixel planes (5,120 bytes per HR pixel) and mode 4's tap buffer are dropped on return."""
    b, _, h, w = feat_c.shape
    packed, image, head = images_on_device(params, mode)
    acts, out, pix = train_buffers(feat_c, hu, wu, _native.load().diinn_initq_pix_bytes(b, wu, hu) // 4)
    with _native.launcher(feat_c.device) as run:
        if mode != 4:
            run("diinn_decode_initq_train_fwd_qonly", feat_c, packed, image, pix, out, acts, b, h, w, hu, wu, int(sin_mode), int(mode == 1))
        else:
            out3 = torch.empty_like(out)                          # the body image's 1x1 head is zero: discarded
            taps = torch.empty(b * hu * wu * TAP_STRIDE, dtype=torch.float32, device=feat_c.device)
            run("diinn_decode_initq_train_fwd", feat_c, packed, image, pix, out3, acts, b, h, w, hu, wu, int(sin_mode))
            run("diinn_head3x3_from_planes", acts, packed, head, taps, out, b, hu, wu)
    return out, acts, packed, image, head


class DecodeInitqModesFunction(torch.autograd.Function):
    """out = decoder(feat) for ``init_q=True`` with mode 1, 2 or 4 on the HIP kernels: differentiable in feat and the 20 parameter
    tensors (INITQ_PARAM_NAMES order, ``param_shapes(mode)``).  The backward needs the saved k_i / s_i planes, the features and the images."""

    @staticmethod
    def forward(ctx, feat: torch.Tensor, hu: int, wu: int, sin_mode: int, mode: int, *params: torch.Tensor) -> torch.Tensor:
        if mode == 4:
            require_2x2(hu, wu)
        feat_c = checked_features(feat, params, INITQ_PARAM_NAMES, param_shapes(mode), hu, wu, PAD_ROWS,
                                  f" for decoder mode {mode} with init_q")
        out, acts, packed, image, head = train_forward_initq_modes(feat_c, params, hu, wu, sin_mode, mode)
        ctx.save_for_backward(feat_c, acts, packed, image, *([head] if head is not None else []))
        ctx.size = (hu, wu)
        ctx.mode = mode
        return out

    @staticmethod
    def backward(ctx, gout: torch.Tensor):
        feat, acts, packed, image, *head = ctx.saved_tensors
        d_feat, d_params = backward_fused_initq_modes(gout.contiguous(), feat, acts, packed, image, ctx.size, ctx.mode,
                                                      head=head[0] if head else None, need_feat_grad=ctx.needs_input_grad[0])
        return function_grads(ctx, d_feat, d_params, 5)


def decode_with_grad(decoder, feat: torch.Tensor, size: Sequence[int]) -> torch.Tensor:
    """``ImplicitDecoder(mode in (1, 2, 4), init_q=True, hip_initq_modes=True, hip_autograd_initq_modes=True).forward(x, size, None)``
    under autograd."""
    hu, wu = size
    return DecodeInitqModesFunction.apply(feat, int(hu), int(wu), int(decoder.sin_mode), int(decoder.mode),
                                          *named_params(decoder, INITQ_PARAM_NAMES))
