"""The LIIF comparison decoder under autograd with the three hidden 256 x 256 layers in split-bf16 arithmetic both ways -- the opt-in
``LIIF.hip_autograd_split_bf16`` together with ``LIIF.hip_autograd`` and ``LIIF.hip_split_bf16``.

The step of ``liif_training.LIIFFunction`` with two kernels exchanged and one image added:

  image     the SPLIT TRAINING image (csrc/diinn_layout.h) of the gathered LIIF image: imnet.layers.{2,4,6}, and their transposes, as
            hi/lo bf16 pieces in the synthesis slots of section WLX's layout, filled on the device (``diinn_pack_split_train``) once
            per weight version and kept beside ``liif_training.image_on_device``'s image under the same key rule (``split_on_device``).
            No new packer, no new format: it is the image ``decoder.pack_liif_split`` builds on the host for inference.
  forward   ``diinn_liif_train_fwd_x3``: the fp32 hoisted conv as before, then liif_x3_save_kernel -- liif_x3_kernel's arithmetic term
            for term (the output under grad is the no_grad split output bit for bit), every 256 x 256 product
            W_lo.h_hi + W_hi.h_lo + W_hi.h_hi on v_mfma_f32_32x32x16_bf16 with fp32 accumulation, hi = bf16(v), lo = bf16(v - hi).  It
            writes the same fp32 planes h_1..h_4 over the virtual pixels as liif_kernel<SAVE>: the unsplit relu(a_l).
  backward  ``liif_training.backward_fused(..., split=image)``: the chain g_a,l-1 = (W_l^T g_a,l) [h_{l-1} > 0] on
            3 x liif_bwd_layer_x3_kernel (``diinn_liif_backward_data_x3``) in the same arithmetic; g_a,4 stays fp32.  The planes it
            leaves are fp32 as before, and everything behind them -- the plane GEMMs, the rowdots, the cell sum, the conv's
            gradients -- is unchanged.

Because the planes keep the fp32 contract the two forwards and the two backwards mix: ``train_forward_split`` +
``liif_training.backward_fused`` without ``split`` is the split forward under the fp32 backward (the tests' bisecting tool).

The EMULATION SHEET (``liif_split_preactivations``, ``liif_split_chain_reference``) states the same arithmetic in torch fp32 on any
device, in the kernels' order of products (the two small ones first, the leading one last); ``liif_backward_from_saved`` is the
formula sheet of ``liif_training.liif_backward_reference`` evaluated on GIVEN activations, in any dtype.  What an end-to-end gradient
comparison cannot hold is the ReLU kink: a pre-activation within the split rounding of zero lands on the other side, and the gate
is discontinuous there.  So the tests pin the gates: the float64 side of a comparison runs on the kernel's own planes, upcast."""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F

from . import _native
from . import liif_training as LT
from . import training as T
from .liif_training import HIDDEN, PARAM_NAMES, PARAM_SHAPES, PLANE_TILE, UNFOLD
from .sheets import split_matmul


# ---------------------------------------------------------------------------
# the split training image
# ---------------------------------------------------------------------------
def split_on_device(params: Sequence[torch.Tensor]) -> torch.Tensor:
    """imnet tensors (PARAM_NAMES order) on a GPU -> the split training image of ``liif_training.image_on_device(params)`` on that GPU
    (``diinn_pack_split_train``).  Kept, like that image, while no parameter has been modified: built once per weight version,
    rebuilt after an optimiser step."""
    def build():
        image = LT.image_on_device(params)
        split = torch.empty(int(_native.load().diinn_split_train_floats()), dtype=torch.float32, device=image.device)
        with _native.launcher(image.device) as run:
            run("diinn_pack_split_train", image, split)
        return split
    return T.kept("liif_split", T.weights_key(params), params, build)


# ---------------------------------------------------------------------------
# forward and the autograd function
# ---------------------------------------------------------------------------
def train_forward_split(feat_c: torch.Tensor, image: torch.Tensor, split: torch.Tensor, hu: int, wu: int
                        ) -> Tuple[torch.Tensor, torch.Tensor]:
    """``diinn_liif_train_fwd_x3`` on a contiguous fp32 CUDA ``feat_c``: (out [B,3,Hu,Wu], acts [4, ceil(4 N / 32), 256, 32] = h_1..h_4
    over the virtual pixels), ``liif_training.train_forward``'s buffers and contract."""
    b, _, h, w = feat_c.shape
    dev = feat_c.device
    out = torch.empty((b, 3, hu, wu), dtype=torch.float32, device=dev)
    acts = torch.empty((4, LT.virtual_tiles(b * hu * wu), HIDDEN, PLANE_TILE), dtype=torch.float32, device=dev)
    workspace = torch.empty(_native.load().diinn_workspace_bytes(b, h, w) // 4, dtype=torch.float32, device=dev)
    with _native.launcher(dev) as run:
        run("diinn_liif_train_fwd_x3", feat_c, image, split, workspace, out, acts, b, h, w, hu, wu)
    return out, acts


class LIIFSplitFunction(torch.autograd.Function):
    """out = LIIF decoder(feat) with the hidden layers in split-bf16 arithmetic both ways, differentiable in feat and the ten imnet
    tensors (PARAM_NAMES order): ``liif_training.LIIFFunction`` on diinn_liif_train_fwd_x3 / diinn_liif_backward_data_x3."""

    @staticmethod
    def forward(ctx, feat: torch.Tensor, hu: int, wu: int, *params: torch.Tensor) -> torch.Tensor:
        feat_c = T.checked_features(feat, params, PARAM_NAMES, PARAM_SHAPES, 4 * hu, wu, HIDDEN)     # the limit counts virtual pixels
        image = LT.image_on_device(params)
        split = split_on_device(params)
        out, acts = train_forward_split(feat_c, image, split, hu, wu)
        ctx.save_for_backward(feat_c, acts, image, split, params[0].detach())
        ctx.size = (hu, wu)
        ctx.wkey = ("liif", params[0].data_ptr(), params[0]._version)
        ctx.wpins = (params[0],)
        return out

    @staticmethod
    def backward(ctx, gout: torch.Tensor):
        feat, acts, image, split, w0 = ctx.saved_tensors
        need = ctx.needs_input_grad
        d_feat, d_params = LT.backward_fused(gout, feat, acts, image, w0, ctx.wkey, ctx.wpins, ctx.size,
                                             need_feat_grad=need[0], need_w0_grad=need[3], split=split)
        return T.function_grads(ctx, d_feat, d_params, 3)


def decode_with_grad(imnet, feat: torch.Tensor, size: Sequence[int]) -> torch.Tensor:
    """``LIIF.query_rgb`` + ``reshape_pred`` of every HR pixel under autograd with ``hip_split_bf16`` and
    ``hip_autograd_split_bf16`` set; ``imnet`` is the model's MLP (modules.MLP)."""
    hu, wu = size
    return LIIFSplitFunction.apply(feat, int(hu), int(wu), *T.named_params(imnet, PARAM_NAMES))


# ---------------------------------------------------------------------------
# the emulation sheet (any device; the CPU tests and DESIGN.md 3.8 cite it)
# ---------------------------------------------------------------------------
def liif_split_preactivations(feat: torch.Tensor, params: Sequence[torch.Tensor], size: Sequence[int]) -> List[torch.Tensor]:
    """a_1..a_4 of the split training forward, each [4 members, N, 256], in torch fp32: layer 1 as
    ``liif_training._forward_parts`` forms it (fp32 in the kernel too), layers 2..4 as ``split_matmul(W_l, h_{l-1}^T)^T + b_l`` on
    h = relu(a) (torch matmuls, not the MFMA's summation order).  relu of these is what liif_x3_save_kernel saves."""
    f32 = torch.float32
    pre1 = LT._forward_parts(feat.detach().to(f32), params, size)[4][0]
    ps = [p.detach().to(device=feat.device, dtype=f32) for p in params]
    pre = [pre1]
    for l in (1, 2, 3):
        ht = torch.relu(pre[-1]).reshape(-1, HIDDEN).t().contiguous()                  # [256, 4 N]
        pre.append((split_matmul(ps[2 * l], ht).t() + ps[2 * l + 1]).reshape(pre1.shape))
    return pre


def liif_split_chain_reference(gout: torch.Tensor, hs: Sequence[torch.Tensor], params: Sequence[torch.Tensor],
                               lr_size: Sequence[int], split: bool = True) -> List[torch.Tensor]:
    """[g_a,4, g_a,3, g_a,2, g_a,1], each [4 members, N, 256], of the backward chain on GIVEN activations ``hs`` = h_1..h_4
    ([4, N, 256] each; every gate is ``h_l > 0``, so a zero or a NaN closes it), in ``gout``'s dtype: g_a,4 = (w_v L^T g) [h_4 > 0] in
    plain algebra (fp32 in the kernel too), and the three transposed products W_l^T g_a,l through ``split_matmul`` as
    liif_bwd_layer_x3_kernel forms them.  ``gout`` [B,3,Hu,Wu]; ``lr_size`` = (H, W) of the feature map (the ensemble weights
    depend on it).  ``split`` false: the same chain with plain products -- in float64, the yardstick of the sheet."""
    dt, dev = gout.dtype, gout.device
    b, _, hu, wu = gout.shape
    n = b * hu * wu
    ps = [p.detach().to(device=dev, dtype=dt) for p in params]
    _, _, wgt = LT._virtual_tables(b, int(lr_size[0]), int(lr_size[1]), hu, wu, dev, dt)
    g = gout.permute(0, 2, 3, 1).reshape(n, 3)
    gh = (wgt.unsqueeze(-1) * g) @ ps[8]                                                # [4, N, 256]
    out = []
    for l in (3, 2, 1):
        ga = gh * (hs[l] > 0)
        out.append(ga)
        gat = ga.reshape(-1, HIDDEN).t().contiguous()                                   # [256 (out), 4 N]
        wt = ps[2 * l].t().contiguous()                                                 # W_l^T [in, out]
        gh = (split_matmul(wt, gat) if split else wt @ gat).t().reshape(ga.shape)
    out.append(gh * (hs[0] > 0))
    return out


def liif_backward_from_saved(gout: torch.Tensor, feat: torch.Tensor, hs: Sequence[torch.Tensor], params: Sequence[torch.Tensor],
                             size: Sequence[int], need_feat_grad: bool = True, chain: Optional[Sequence[torch.Tensor]] = None
                             ) -> Tuple[Optional[torch.Tensor], List[torch.Tensor]]:
    """The formula sheet of ``liif_training.liif_backward_reference`` evaluated on GIVEN activations ``hs`` = h_1..h_4 ([4 members, N,
    256] each; the masks are ``h_l > 0``) instead of a forward of its own, in ``gout``'s dtype: with the kernel's own planes upcast,
    the float64 side of a comparison whose gates are pinned (mode 3 has ``training.backward_from_saved`` for this).
    ``chain`` ([g_a,4 .. g_a,1], e.g. ``liif_split_chain_reference``'s): used in the place of the plain chain.
    Returns (d feat or None, [d param ...] in PARAM_NAMES order)."""
    dt, dev = gout.dtype, gout.device
    feat = feat.detach().to(device=dev, dtype=dt)
    b, c, h, w = feat.shape
    hu, wu = int(size[0]), int(size[1])
    n = b * hu * wu
    ps = [p.detach().to(device=dev, dtype=dt) for p in params]
    hs = [h_.to(device=dev, dtype=dt) for h_ in hs]
    cell, r, wgt = LT._virtual_tables(b, h, w, hu, wu, dev, dt)
    u = F.unfold(feat, 3, padding=1).permute(0, 2, 1).reshape(b * h * w, c * 9)
    if chain is None:
        chain = liif_split_chain_reference(gout, hs, ps, (h, w), split=False)
    ga = {4 - i: g_.to(device=dev, dtype=dt) for i, g_ in enumerate(chain)}             # l -> g_a,l
    g = gout.permute(0, 2, 3, 1).reshape(n, 3)
    wg = wgt.unsqueeze(-1) * g                                                          # [4, N, 3]
    d_wl = torch.einsum("vpk,vpj->kj", wg, hs[3])
    d_bl = wg.sum((0, 1))
    grads: List[torch.Tensor] = []
    for l in (2, 3, 4):                                                                 # imnet.layers.{2,4,6}
        grads += [torch.einsum("vpo,vpi->oi", ga[l], hs[l - 2]), ga[l].sum((0, 1))]
    d_wc = torch.einsum("vpo,vpk->ok", ga[1], r)
    d_p1 = torch.zeros((b * h * w, HIDDEN), dtype=dt, device=dev).index_add_(0, cell.reshape(-1), ga[1].reshape(4 * n, HIDDEN))
    d_w0 = torch.cat([d_p1.t() @ u, d_wc], dim=1)
    d_b0 = d_p1.sum(0)
    d_feat = None
    if need_feat_grad:
        du = d_p1 @ ps[0][:, :UNFOLD]
        d_feat = F.fold(du.view(b, h * w, c * 9).permute(0, 2, 1), (h, w), 3, padding=1)
    return d_feat, [d_w0, d_b0, *grads, d_wl, d_bl]
