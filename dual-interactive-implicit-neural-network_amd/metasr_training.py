"""Training path of the MetaSR comparison decoder: autograd through the HIP kernels.

The reference trains MetaSR by ``forward(lr, size, None)`` under autograd (sr_module.py:42-48,127-129 -> metasr.py:125-132 ->
``query_rgb``, :70-104), which materialises the predicted filters ``pred`` [B*Hu*Wu, 1728] and their gradient.  Here the
backward pass collapses onto the LR cells.  Per HR pixel p with cell c(p), inp = (rel_h, rel_w, r_rev):

    a = W1 inp + b1,   h = relu(a),   pred = W2 h + b2 (index 3 n + comp, n = ch*9 + 3 ky + kx),
    out[comp] = sum_n U[c][n] pred[3 n + comp],   U = unfold3x3(feat).

Hoisted form, with W2r[n, comp, j] = W2[3 n + comp, j]:

    M[c][comp][j] = sum_n W2r[n, comp, j] U[c][n],   B0[c][comp] = sum_n b2[3 n + comp] U[c][n],
    out[comp] = sum_j h_j M[c][comp][j] + B0[c][comp]:

[M; B0] is a 3x3 convolution of the feature map with 771 outputs -- DIINN's hoisted conv P under another weight.  With
g = d loss / d out:

    dh_p = sum_comp g_p[comp] M[c][comp][:],  da_p = dh_p [a_p > 0],  dW1 = sum_p da_p (x) inp_p,  db1 = sum_p da_p,
    S[c][comp][j] = sum over the cell's pixels of g_p[comp] h_p[j]  (= dM),    G[c][comp] = sum of g_p[comp]  (= dB0),
    dW2r[n, comp, j] = sum_c U[c][n] S[c][comp][j],   db2[3 n + comp] = sum_c U[c][n] G[c][comp],
    d_feat = conv3x3([S; G]; the conv's weight transposed and flipped).

  forward   the inference kernels (``metasr_decode_features``: the output under grad is the no_grad output bit for bit),
            plus M on ``diinn_precompute_P_wpu`` from a training image gathered on the device.  With ``MetaSR.hip_hoisted`` the
            output comes from that M instead (``metasr_decode_hoisted``, again the no_grad call itself): metasr_kernel is not run.
  backward  ``metasr_bwd_cells_kernel`` (C ABI ``diinn_metasr_backward_cells``): everything per pixel, leaving [S; G] in both of
            cell_sum_kernel's layouts and the layer-0 partials; then ``training._conv_grads_native`` -- unfold + plane GEMM for
            dW2 / db2, the encoder's convolution kernels for d_feat -- and ``diinn_sum_parts``.  No framework convolution or GEMM.
  ``metasr_backward_reference`` states the same gradients in device-agnostic tensor algebra: the formula sheet, tested on the
  CPU against the reference's own .grad fixtures, and the on-GPU cross-check of the fused path (float64).

The conv is embedded in the 1024-row shape the DIINN kernels take: rows 256 comp + j hold W2r[:, comp, j] as a [64,3,3] filter,
row 768 + comp holds b2[:, comp], every other row and every bias is zero.
"""
from __future__ import annotations

import functools
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from . import _native
from . import training as T

HIDDEN = T.HIDDEN
UNFOLD = T.UNFOLD
ROWS = 4 * HIDDEN                                            # rows of the embedded conv (771 used)
PARAM_NAMES: List[str] = ["layers.0.weight", "layers.0.bias", "layers.2.weight", "layers.2.bias"]
PARAM_SHAPES: Dict[str, Tuple[int, ...]] = {"layers.0.weight": (HIDDEN, 3), "layers.0.bias": (HIDDEN,),
                                            "layers.2.weight": (3 * UNFOLD, HIDDEN), "layers.2.bias": (3 * UNFOLD,)}


# ---------------------------------------------------------------------------
# the formula sheet (device-agnostic, any floating dtype)
# ---------------------------------------------------------------------------
def _pixel_tables(b: int, h: int, w: int, hu: int, wu: int, device, dtype):
    """Per HR pixel of the flattened (b, y, x) index: its cell (b*H + cy)*W + cx and inp = (rel_h, rel_w, r_rev), from the host
    tables of the C ABI (bit-exact with metasr_kernel; cast to ``dtype``)."""
    from .decoder import metasr_axis_tables
    idx_h, rel_h, r_rev = metasr_axis_tables(h, hu)
    idx_w, rel_w, _ = metasr_axis_tables(w, wu)
    iy = torch.from_numpy(idx_h.astype(np.int64)).to(device)
    ix = torch.from_numpy(idx_w.astype(np.int64)).to(device)
    cell = ((torch.arange(b, device=device).view(b, 1, 1) * h + iy.view(1, hu, 1)) * w + ix.view(1, 1, wu)).reshape(-1)
    inp = torch.empty((b, hu, wu, 3), dtype=dtype, device=device)
    inp[..., 0] = torch.from_numpy(rel_h).to(device=device, dtype=dtype).view(1, hu, 1)
    inp[..., 1] = torch.from_numpy(rel_w).to(device=device, dtype=dtype).view(1, 1, wu)
    inp[..., 2] = float(r_rev)
    return cell, inp.view(-1, 3)


def _hoisted(feat: torch.Tensor, w2: torch.Tensor, b2: torch.Tensor):
    """U [cells,576], W2r [576,3,256], b2r [576,3], M [cells,3,256], B0 [cells,3]."""
    b, c, h, w = feat.shape
    u = F.unfold(feat, 3, padding=1).permute(0, 2, 1).reshape(b * h * w, c * 9)
    w2r = w2.reshape(c * 9, 3, HIDDEN)
    b2r = b2.reshape(c * 9, 3)
    return u, w2r, b2r, torch.einsum("cn,nkj->ckj", u, w2r), u @ b2r


def metasr_forward_reference(feat: torch.Tensor, params: Sequence[torch.Tensor], size: Sequence[int]) -> torch.Tensor:
    """out [B,3,Hu,Wu] of the MetaSR decoder in the hoisted form (module docstring), in ``feat``'s dtype."""
    dt = feat.dtype
    w1, b1, w2, b2 = (p.detach().to(dt) for p in params)
    b, _, h, w = feat.shape
    hu, wu = int(size[0]), int(size[1])
    cell, inp = _pixel_tables(b, h, w, hu, wu, feat.device, dt)
    _, _, _, m, b0 = _hoisted(feat, w2, b2)
    hid = torch.relu(inp @ w1.t() + b1)
    out = torch.einsum("pj,pkj->pk", hid, m[cell]) + b0[cell]
    return out.view(b, hu, wu, 3).permute(0, 3, 1, 2).contiguous()


def metasr_backward_reference(gout: torch.Tensor, feat: torch.Tensor, params: Sequence[torch.Tensor], size: Sequence[int],
                              need_feat_grad: bool = True) -> Tuple[Optional[torch.Tensor], List[torch.Tensor]]:
    """Gradients of the MetaSR decoder given d(loss)/d(out): the formula sheet of the module docstring in plain tensor ops.
    gout [B,3,Hu,Wu]; feat [B,64,H,W]; params in PARAM_NAMES order.  Everything is computed in ``gout``'s dtype.
    Returns (d feat or None, [d param ...] in PARAM_NAMES order)."""
    dt = gout.dtype
    feat = feat.detach().to(dt)
    w1, b1, w2, b2 = (p.detach().to(dt) for p in params)
    b, c, h, w = feat.shape
    hu, wu = int(size[0]), int(size[1])
    cells = b * h * w
    cell, inp = _pixel_tables(b, h, w, hu, wu, feat.device, dt)
    u, w2r, b2r, m, _ = _hoisted(feat, w2, b2)
    g = gout.permute(0, 2, 3, 1).reshape(-1, 3)
    a = inp @ w1.t() + b1
    hid = torch.relu(a)
    dh = torch.einsum("pk,pkj->pj", g, m[cell])
    da = dh * (a > 0)
    d_w1 = da.t() @ inp
    d_b1 = da.sum(0)
    s = torch.zeros((cells, 3, HIDDEN), dtype=dt, device=feat.device).index_add_(0, cell, g.unsqueeze(2) * hid.unsqueeze(1))
    gs = torch.zeros((cells, 3), dtype=dt, device=feat.device).index_add_(0, cell, g)
    d_w2 = torch.einsum("cn,ckj->nkj", u, s).reshape(3 * c * 9, HIDDEN)
    d_b2 = (u.t() @ gs).reshape(3 * c * 9)
    d_feat = None
    if need_feat_grad:
        du = torch.einsum("ckj,nkj->cn", s, w2r) + gs @ b2r.t()
        d_feat = F.fold(du.view(b, h * w, c * 9).permute(0, 2, 1), (h, w), 3, padding=1)
    return d_feat, [d_w1, d_b1, d_w2, d_b2]


# ---------------------------------------------------------------------------
# images gathered on the device (the weights change every optimiser step: no host packing inside the step)
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def conv_gather_index() -> torch.Tensor:
    """int64 [1024*576]: Wx.flatten()[i] = flat[index[i]] for the embedded conv weight Wx [1024,64,3,3], where ``flat`` is
    (layers.2.weight [1728,256], layers.2.bias [1728]) flattened, followed by one 0.0:
        Wx[256 comp + j, n] = W2[3 n + comp, j],    Wx[768 + comp, n] = b2[3 n + comp],    zero elsewhere."""
    nw = 3 * UNFOLD * HIDDEN
    idx = np.full((ROWS, UNFOLD), nw + 3 * UNFOLD, dtype=np.int64)                # the appended zero
    n = np.arange(UNFOLD, dtype=np.int64)
    j = np.arange(HIDDEN, dtype=np.int64)
    for comp in range(3):
        idx[HIDDEN * comp:HIDDEN * (comp + 1)] = (3 * n[None, :] + comp) * HIDDEN + j[:, None]
        idx[3 * HIDDEN + comp] = nw + 3 * n + comp
    return torch.from_numpy(idx.reshape(-1))


@functools.lru_cache(maxsize=None)
def pack_gather_index() -> torch.Tensor:
    """int64 [MetaSR packed floats]: packed[i] = flat[index[i]] with ``flat`` the four imnet tensors flattened in PARAM_NAMES
    order.  Derived by packing a state dict whose values are their own flat position (exact in fp32); the MetaSR image is a
    pure permutation of its parameters (no padding, no appended zero: a stricter rule than ``training.gather_index``'s)."""
    from .decoder import pack_metasr_state_dict
    sd, total = T.position_state_dict(PARAM_NAMES, PARAM_SHAPES)
    idx = np.rint(pack_metasr_state_dict(sd, prefix="").numpy()).astype(np.int64) - 1
    if idx.min() < 0 or idx.max() >= total or np.unique(idx).size != total or idx.size != total:
        raise RuntimeError("the MetaSR packed image is not a permutation of the imnet tensors")
    return torch.from_numpy(idx)


def conv_weight_on_device(w2: torch.Tensor, b2: torch.Tensor) -> torch.Tensor:
    """The embedded conv weight Wx [1024,64,3,3] (``conv_gather_index``) on the tensors' device: one gather."""
    dev = w2.device
    flat = torch.cat([w2.detach().reshape(-1).to(torch.float32), b2.detach().reshape(-1).to(torch.float32), torch.zeros(1, device=dev)])
    return flat.index_select(0, T.index_on(dev, "metasr conv", conv_gather_index)).view(ROWS, T.IN_CHANNELS, 3, 3)


def images_on_device(params: Sequence[torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """imnet tensors (PARAM_NAMES order) on a GPU -> (the MetaSR packed image metasr_kernel reads, the DIINN-shaped training
    image whose section 13 holds the embedded conv in Winograd form -- what diinn_precompute_P_wpu reads; every bias zero --,
    the embedded conv weight Wx).  Kept while no parameter has been modified (a training step decodes once per scale)."""
    def build():
        w1, b1, w2, b2 = params
        dev = w2.device
        flat = torch.cat([p.detach().reshape(-1).to(torch.float32) for p in params])
        packed = flat.index_select(0, T.index_on(dev, "metasr pack", pack_gather_index))
        wx = conv_weight_on_device(w2, b2)
        image = torch.zeros(_native.load().diinn_packed_weight_floats(), dtype=torch.float32, device=dev)
        T._fill_wpu_weight(image, wx)
        return packed, image, wx
    return T.kept("metasr", T.weights_key(params), params, build)


# ---------------------------------------------------------------------------
# the fused backward
# ---------------------------------------------------------------------------
_seg_cache: "Dict[tuple, Tuple[torch.Tensor, torch.Tensor]]" = {}


def cell_segments(h: int, w: int, hu: int, wu: int, dev) -> Tuple[torch.Tensor, torch.Tensor]:
    """seg_h [H+1] / seg_w [W+1] (int32, on ``dev``): the first HR row / column of every LR row / column of MetaSR's index table
    (monotone), last entry Hu / Wu.  One entry per (LR size, HR size, device) of a training run."""
    from .decoder import metasr_axis_tables

    def build():
        idx_h, idx_w = metasr_axis_tables(h, hu)[0], metasr_axis_tables(w, wu)[0]
        if (np.diff(idx_h) < 0).any() or (np.diff(idx_w) < 0).any():
            raise RuntimeError("MetaSR's index table is not monotone")
        return (torch.from_numpy(np.searchsorted(idx_h, np.arange(h + 1)).astype(np.int32)).to(dev),
                torch.from_numpy(np.searchsorted(idx_w, np.arange(w + 1)).astype(np.int32)).to(dev))
    return T.lru(_seg_cache, (h, w, hu, wu, str(dev)), build)


def backward_cells(gout: torch.Tensor, m: torch.Tensor, packed: torch.Tensor, size: Sequence[int]):
    """``diinn_metasr_backward_cells`` on contiguous fp32 CUDA tensors: gout [B,3,Hu,Wu], m [B,H,W,1024], packed the MetaSR image.
    Returns (dM NCHW [B,1024,H,W], dM tiled over cells [T,1024,32], [dW1 | db1] [256,4])."""
    b, h, w, _ = m.shape
    hu, wu = int(size[0]), int(size[1])
    dev = gout.device
    tc = (b * h * w + T.PLANE_TILE - 1) // T.PLANE_TILE
    seg_h, seg_w = cell_segments(h, w, hu, wu, dev)
    dm = torch.empty((b, ROWS, h, w), dtype=torch.float32, device=dev)
    dm_t = torch.empty((tc, ROWS, T.PLANE_TILE), dtype=torch.float32, device=dev)
    part0 = torch.empty((2 * tc, HIDDEN, 4), dtype=torch.float32, device=dev)
    with _native.launcher(dev) as run:
        run("diinn_metasr_backward_cells", gout, m, packed, seg_h, seg_w, dm, dm_t, part0, b, h, w, hu, wu)
    d0 = T._sum_parts(part0.view(1, 2 * tc, HIDDEN * 4)).view(HIDDEN, 4)
    return dm, dm_t, d0


def backward_fused(gout: torch.Tensor, feat: torch.Tensor, m: torch.Tensor, packed: torch.Tensor, wx, wkey, wpins,
                   size: Sequence[int], need_feat_grad: bool = True, need_w2_grad: bool = True
                   ) -> Tuple[Optional[torch.Tensor], List[Optional[torch.Tensor]]]:
    """The same gradients as ``metasr_backward_reference``, on the HIP kernels throughout.  ``wx``: the embedded conv weight or a
    callable returning it; ``wkey`` / ``wpins`` identify its values for the cache of the transposed weight."""
    dm, dm_t, d0 = backward_cells(gout.to(torch.float32).contiguous(), m, packed, size)
    d_wx, d_feat = T._conv_grads_native(feat, wx, dm, need_feat_grad, want_weight=need_w2_grad, wkey=wkey, wpins=wpins, a_t=dm_t, rows=ROWS)
    d_w2 = d_b2 = None
    if need_w2_grad:                                             # d_wx [1024, 576]: rows 256 comp + j -> W2[3 n + comp, j]; rows 768 + comp -> b2
        d_w2 = d_wx[:3 * HIDDEN].reshape(3, HIDDEN, UNFOLD).permute(2, 0, 1).reshape(3 * UNFOLD, HIDDEN)
        d_b2 = d_wx[3 * HIDDEN:3 * HIDDEN + 3].t().reshape(3 * UNFOLD)
    return d_feat, [d0[:, :3].contiguous(), d0[:, 3].contiguous(), d_w2, d_b2]


def _function_forward(ctx, hoisted: bool, feat: torch.Tensor, hu: int, wu: int, params: Sequence[torch.Tensor]) -> torch.Tensor:
    from .decoder import metasr_decode_features, metasr_decode_hoisted
    feat_c = T.checked_features(feat, params, PARAM_NAMES, PARAM_SHAPES, hu, wu, ROWS)
    b, _, h, w = feat_c.shape
    packed, image, wx = images_on_device(params)
    if hoisted:                                                  # the inference call itself: M into m, the pixels from m
        m = torch.empty((b, h, w, ROWS), dtype=torch.float32, device=feat_c.device)
        out = metasr_decode_hoisted(feat_c, packed, image, (hu, wu), workspace=m.view(-1))
    else:
        out = metasr_decode_features(feat_c, packed, (hu, wu))
        m = torch.empty((b, h, w, ROWS), dtype=torch.float32, device=feat_c.device)
        with _native.launcher(feat_c.device) as run:
            run("diinn_precompute_P_wpu", feat_c, image, m, b, h, w, 0, h)
    ctx.save_for_backward(feat_c, m, packed, wx)
    ctx.size = (hu, wu)
    ctx.wkey = ("metasr", *((p_.data_ptr(), p_._version) for p_ in params[2:]))
    ctx.wpins = tuple(params[2:])
    return out


class MetaSRFunction(torch.autograd.Function):
    """out = MetaSR decoder(feat) on the HIP kernels, differentiable in feat and the four imnet tensors (PARAM_NAMES order)."""

    @staticmethod
    def forward(ctx, feat: torch.Tensor, hu: int, wu: int, *params: torch.Tensor) -> torch.Tensor:
        return _function_forward(ctx, False, feat, hu, wu, params)

    @staticmethod
    def backward(ctx, gout: torch.Tensor):
        feat, m, packed, wx = ctx.saved_tensors
        need = ctx.needs_input_grad
        d_feat, d_params = backward_fused(gout, feat, m, packed, wx, ctx.wkey, ctx.wpins, ctx.size,
                                          need_feat_grad=need[0], need_w2_grad=need[5] or need[6])
        return T.function_grads(ctx, d_feat, d_params, 3)


class MetaSRHoistedFunction(MetaSRFunction):
    """The same function with the forward in the hoisted form (``decoder.metasr_decode_hoisted``: M by diinn_precompute_P_wpu as
    above, the output from M by diinn_metasr_decode_hoisted; diinn_metasr_decode is not launched).  The backward is the same."""

    @staticmethod
    def forward(ctx, feat: torch.Tensor, hu: int, wu: int, *params: torch.Tensor) -> torch.Tensor:
        return _function_forward(ctx, True, feat, hu, wu, params)


def decode_with_grad(imnet, feat: torch.Tensor, size: Sequence[int], hoisted: bool = False) -> torch.Tensor:
    """``MetaSR.query_rgb`` + ``reshape_pred`` of every HR pixel under autograd; ``imnet`` is the model's meta-network (modules.MLP)."""
    hu, wu = size
    fn = MetaSRHoistedFunction if hoisted else MetaSRFunction
    return fn.apply(feat, int(hu), int(wu), *T.named_params(imnet, PARAM_NAMES))
