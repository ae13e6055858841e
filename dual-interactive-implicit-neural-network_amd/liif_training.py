"""Training path of the LIIF comparison decoder: autograd through the HIP kernels.  Opt-in: ``LIIF.hip_autograd``.

The reference trains LIIF by ``forward(lr, size, None)`` under autograd (sr_module.py:42-48,127-129 -> liif.py:148-155 ->
``query_rgb``, :59-127).  Per HR pixel p and ensemble member v = 2 vh + vw (vx outer, vy inner, liif.py:88-89), with
c_v(p) = (iy[vh], ix[vw]) the shifted nearest cell and r_v = (rel_h[vh], rel_w[vw], cell_h, cell_w) (no gradient flows into a
coordinate):

    a_1 = P1[c_v] + Wc r_v            P1 = conv3x3(feat; W0[:, :576]) + b0 (the hoisted first layer),   Wc = W0[:, 576:580]
    h_1 = relu(a_1)    a_l = W_l h_{l-1} + b_l,  h_l = relu(a_l)   (l = 2, 3, 4: imnet.layers.{2,4,6})
    pred_v = L h_4 + bL               out = sum_v w_v pred_v,   w_v = area[3 - v] / tot   (liif.py:117-126)

With g = d loss / d out:

    g_h,4 = w_v L^T g                 g_a,l = g_h,l [a_l > 0]          g_h,l-1 = W_l^T g_a,l
    dL = sum_{p,v} w_v g (x) h_4      dbL = sum_{p,v} w_v g
    dW_l = sum_{p,v} g_a,l (x) h_{l-1}  db_l = sum_{p,v} g_a,l         (l = 2..4)
    dWc = sum_{p,v} g_a,1 (x) r_v     dP1[cell] = sum over (p, v) with c_v(p) = cell of g_a,1
    db0 = sum over cells of dP1       dW0[:, :576], d_feat: the hoisted conv's gradients from dP1

The pairs (p, v) are the VIRTUAL pixels vp = v * N + p (N = B Hu Wu); every plane group of this path is tiled over them,
[ceil(4 N / 32)][256][32].

  forward   ``diinn_liif_train_fwd``: the inference forward's two kernels on the same image -- the output under grad is the no_grad
            output bit for bit -- with liif_kernel<SAVE> writing h_1..h_4 of every member (a post-ReLU value is its own mask).
  backward  ``diinn_liif_backward_data`` (3 x liif_bwd_layer_kernel: the chain g_a,4 .. g_a,1), ``diinn_plane_gemm_nt`` for
            [dW_l | db_l], ``diinn_plane_rowdot`` for dL (against w_v g) and [dWc | db0] (against (rel_h, rel_w, 1, 0): cell_h and
            cell_w are constant, so two columns of dWc are the row sum scaled), ``diinn_liif_cell_sum`` for dP1 in both of
            cell_sum_kernel's layouts, then ``training._conv_grads_native`` with rows = 256 and ``diinn_sum_parts``.
            No framework convolution or GEMM.  dbL is taken as sum_p g (the four weights of a pixel add up to 1 up to rounding).
  ``liif_backward_reference`` states the same gradients in device-agnostic tensor algebra: the formula sheet, tested on the CPU
  against the reference's own .grad fixtures, and the on-GPU cross-check of the fused path (float64, given the forward's masks).

One image serves the whole step: the inference image gathered on the device (``pack_gather_index``); liif_kernel, the direct hoisted
conv (its section WP) and the backward (sections WLT, L) read permutation sections only.  The Winograd training image of the
other training paths is not used: P must be the inference forward's, bit for bit.
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
PLANE_TILE = T.PLANE_TILE
PARAM_NAMES: List[str] = [f"layers.{i}.{t}" for i in (0, 2, 4, 6, 8) for t in ("weight", "bias")]
PARAM_SHAPES: Dict[str, Tuple[int, ...]] = {
    "layers.0.weight": (HIDDEN, UNFOLD + 4), "layers.0.bias": (HIDDEN,),
    **{f"layers.{i}.weight": (HIDDEN, HIDDEN) for i in (2, 4, 6)}, **{f"layers.{i}.bias": (HIDDEN,) for i in (2, 4, 6)},
    "layers.8.weight": (3, HIDDEN), "layers.8.bias": (3,),
}


# ---------------------------------------------------------------------------
# the formula sheet (device-agnostic, any floating dtype)
# ---------------------------------------------------------------------------
def _axis_tables(h: int, w: int, hu: int, wu: int):
    """Host tables of the C ABI (bit-exact with liif_kernel): per shift (-1, +1) and axis (idx int32, rel fp32), and (cell_h, cell_w)."""
    from .decoder import liif_axis_tables
    th = [liif_axis_tables(h, hu, s) for s in (-1, 1)]
    tw = [liif_axis_tables(w, wu, s) for s in (-1, 1)]
    return th, tw, (float(th[0][2]), float(tw[0][2]))


def _virtual_tables(b: int, h: int, w: int, hu: int, wu: int, device, dtype):
    """Per member v and HR pixel of the flattened (b, y, x) index: cell [4, N] (int64, (b*H + iy)*W + ix), r [4, N, 4] =
    (rel_h, rel_w, cell_h, cell_w) and the ensemble weight w_v [4, N] = area[3 - v] / tot, the tables cast to ``dtype``."""
    th, tw, (cell_h, cell_w) = _axis_tables(h, w, hu, wu)
    n = b * hu * wu
    cells, rs, areas = [], [], []
    bi = torch.arange(b, device=device).view(b, 1, 1)
    for v in range(4):
        idx_h, rel_h, _ = th[v >> 1]
        idx_w, rel_w, _ = tw[v & 1]
        iy = torch.from_numpy(idx_h.astype(np.int64)).to(device).view(1, hu, 1)
        ix = torch.from_numpy(idx_w.astype(np.int64)).to(device).view(1, 1, wu)
        cells.append(((bi * h + iy) * w + ix).reshape(-1))
        rh = torch.from_numpy(rel_h).to(device=device, dtype=dtype).view(1, hu, 1).expand(b, hu, wu)
        rw = torch.from_numpy(rel_w).to(device=device, dtype=dtype).view(1, 1, wu).expand(b, hu, wu)
        r = torch.empty((b, hu, wu, 4), dtype=dtype, device=device)
        r[..., 0] = rh
        r[..., 1] = rw
        r[..., 2] = cell_h
        r[..., 3] = cell_w
        rs.append(r.view(n, 4))
        areas.append(((rh * rw).abs() + 1e-9).reshape(n))
    tot = ((areas[0] + areas[1]) + areas[2]) + areas[3]
    wgt = torch.stack([areas[3 - v] / tot for v in range(4)])
    return torch.stack(cells), torch.stack(rs), wgt


def _forward_parts(feat: torch.Tensor, params: Sequence[torch.Tensor], size: Sequence[int]):
    """(u [cells,576], cell, r, wgt, [a_1..a_4] each [4, N, 256], the ten tensors) in ``feat``'s dtype."""
    dt = feat.dtype
    ps = [p.detach().to(dt) for p in params]
    w0, b0 = ps[0], ps[1]
    b, c, h, w = feat.shape
    hu, wu = int(size[0]), int(size[1])
    cell, r, wgt = _virtual_tables(b, h, w, hu, wu, feat.device, dt)
    u = F.unfold(feat, 3, padding=1).permute(0, 2, 1).reshape(b * h * w, c * 9)
    p1 = u @ w0[:, :UNFOLD].t() + b0
    pre = [p1[cell] + r @ w0[:, UNFOLD:].t()]
    for l in (1, 2, 3):
        pre.append(torch.relu(pre[-1]) @ ps[2 * l].t() + ps[2 * l + 1])
    return u, cell, r, wgt, pre, ps


def liif_preactivations(feat: torch.Tensor, params: Sequence[torch.Tensor], size: Sequence[int]) -> List[torch.Tensor]:
    """a_1..a_4, each [4 members, N, 256], in ``feat``'s dtype (what a test looks at the ReLU kink with)."""
    return _forward_parts(feat, params, size)[4]


def liif_forward_reference(feat: torch.Tensor, params: Sequence[torch.Tensor], size: Sequence[int]) -> torch.Tensor:
    """out [B,3,Hu,Wu] of the LIIF decoder in the hoisted form (module docstring), in ``feat``'s dtype."""
    _, _, _, wgt, pre, ps = _forward_parts(feat, params, size)
    pred = torch.relu(pre[3]) @ ps[8].t() + ps[9]                 # [4, N, 3]
    out = 0
    for v in range(4):                                            # the reference's order of the blend (liif.py:124-126)
        out = out + pred[v] * wgt[v].unsqueeze(-1)
    b = feat.shape[0]
    return out.view(b, int(size[0]), int(size[1]), 3).permute(0, 3, 1, 2).contiguous()


def liif_backward_reference(gout: torch.Tensor, feat: torch.Tensor, params: Sequence[torch.Tensor], size: Sequence[int],
                            need_feat_grad: bool = True, masks: Optional[Sequence[torch.Tensor]] = None
                            ) -> Tuple[Optional[torch.Tensor], List[torch.Tensor]]:
    """Gradients of the LIIF decoder given d(loss)/d(out): the formula sheet of the module docstring in plain tensor ops.
    gout [B,3,Hu,Wu]; feat [B,64,H,W]; params in PARAM_NAMES order.  Everything is computed in ``gout``'s dtype.
    ``masks`` (four bool tensors [4 members, N, 256], layers 1..4), when given, replace [a_l > 0].
    Returns (d feat or None, [d param ...] in PARAM_NAMES order)."""
    dt = gout.dtype
    feat = feat.detach().to(dt)
    b, c, h, w = feat.shape
    hu, wu = int(size[0]), int(size[1])
    n = b * hu * wu
    u, cell, r, wgt, pre, ps = _forward_parts(feat, params, size)
    if masks is None:
        masks = [a > 0 for a in pre]
    hs = [torch.relu(a) for a in pre]
    w0 = ps[0]
    g = gout.permute(0, 2, 3, 1).reshape(n, 3)
    wg = wgt.unsqueeze(-1) * g                                    # [4, N, 3]
    d_wl = torch.einsum("vpk,vpj->kj", wg, hs[3])
    d_bl = wg.sum((0, 1))
    gh = wg @ ps[8]                                               # [4, N, 256]
    d_w: List[Optional[torch.Tensor]] = [None] * 4
    d_b: List[Optional[torch.Tensor]] = [None] * 4
    for l in (3, 2, 1):
        ga = gh * masks[l]
        d_w[l] = torch.einsum("vpo,vpi->oi", ga, hs[l - 1])
        d_b[l] = ga.sum((0, 1))
        gh = ga @ ps[2 * l]
    ga = gh * masks[0]
    d_wc = torch.einsum("vpo,vpk->ok", ga, r)
    d_p1 = torch.zeros((b * h * w, HIDDEN), dtype=dt, device=feat.device).index_add_(0, cell.reshape(-1), ga.reshape(4 * n, HIDDEN))
    d_w0 = torch.cat([d_p1.t() @ u, d_wc], dim=1)
    d_b0 = d_p1.sum(0)
    d_feat = None
    if need_feat_grad:
        du = d_p1 @ w0[:, :UNFOLD]
        d_feat = F.fold(du.view(b, h * w, c * 9).permute(0, 2, 1), (h, w), 3, padding=1)
    return d_feat, [d_w0, d_b0, d_w[1], d_b[1], d_w[2], d_b[2], d_w[3], d_b[3], d_wl, d_bl]


# ---------------------------------------------------------------------------
# the image gathered on the device (the weights change every optimiser step: no host packing inside the step)
# ---------------------------------------------------------------------------
DERIVED_SECTIONS = T.DERIVED_SECTIONS                          # inference-only sections of the DIINN image: derived values, no gather


@functools.lru_cache(maxsize=None)
def pack_gather_index() -> torch.Tensor:
    """int64 [packed floats]: packed[i] = flat[index[i]] with ``flat`` the ten imnet tensors flattened in PARAM_NAMES order followed
    by one 0.0.  Derived by packing a state dict whose values are their own flat position (exact in fp32) through
    ``pack_liif_state_dict``.  The places LIIF leaves empty (the modulation slots), the derived sections -- no LIIF kernel
    reads them -- and the validity word point at the appended zero; every parameter element is referenced."""
    from .decoder import pack_liif_state_dict
    sd, total = T.position_state_dict(PARAM_NAMES, PARAM_SHAPES)
    return T.gather_index(pack_liif_state_dict(sd, prefix="").numpy(), total, T.derived_ranges(), "the LIIF packed image", of="imnet")


def image_on_device(params: Sequence[torch.Tensor]) -> torch.Tensor:
    """imnet tensors (PARAM_NAMES order) on a GPU -> the packed image on that GPU: one ``index_select``.  Kept while no parameter
    has been modified (a training step decodes once per scale with the same weights)."""
    def build():
        dev = params[0].device
        flat = torch.cat([p.detach().reshape(-1).to(torch.float32) for p in params] + [torch.zeros(1, device=dev)])
        return flat.index_select(0, T.index_on(dev, "liif", pack_gather_index))
    return T.kept("liif", T.weights_key(params), params, build)


# ---------------------------------------------------------------------------
# forward with saved planes, fused backward
# ---------------------------------------------------------------------------
def virtual_tiles(n: int) -> int:
    return (4 * n + PLANE_TILE - 1) // PLANE_TILE


def train_forward(feat_c: torch.Tensor, image: torch.Tensor, hu: int, wu: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """``diinn_liif_train_fwd`` on a contiguous fp32 CUDA ``feat_c``: (out [B,3,Hu,Wu], acts [4, ceil(4 N / 32), 256, 32] = h_1..h_4 over
    the virtual pixels)."""
    b, _, h, w = feat_c.shape
    dev = feat_c.device
    out = torch.empty((b, 3, hu, wu), dtype=torch.float32, device=dev)
    acts = torch.empty((4, virtual_tiles(b * hu * wu), HIDDEN, PLANE_TILE), dtype=torch.float32, device=dev)
    workspace = torch.empty(_native.load().diinn_workspace_bytes(b, h, w) // 4, dtype=torch.float32, device=dev)
    with _native.launcher(dev) as run:
        run("diinn_liif_train_fwd", feat_c, image, workspace, out, acts, b, h, w, hu, wu)
    return out, acts


def saved_activations(acts: torch.Tensor, b: int, hu: int, wu: int) -> torch.Tensor:
    """The forward's tiled planes as [4 members][4 layers][256][B Hu Wu] (a copy; tests)."""
    n = b * hu * wu
    return T.untile_planes(acts, 4 * n).reshape(4, HIDDEN, 4, n).permute(2, 0, 1, 3).contiguous()


_geo_cache: "Dict[tuple, dict]" = {}


def _geometry(b: int, h: int, w: int, hu: int, wu: int, dev) -> dict:
    """Per-shape constants of the backward pass, built once per (B, LR size, HR size, device) like ``training._geometry``: the
    members' cell rectangles (seg_h [2, H+1], seg_w [2, W+1]; each index table must be monotone), the ensemble weights over the
    virtual pixels and the tiled right-hand side (rel_h, rel_w, 1, 0) of the layer-1 product."""
    def build():
        th, tw, (cell_h, cell_w) = _axis_tables(h, w, hu, wu)
        for idx, _, _ in th + tw:
            if (np.diff(idx) < 0).any():
                raise RuntimeError("LIIF's index table is not monotone")
        seg_h = np.stack([np.searchsorted(th[s][0], np.arange(h + 1)) for s in (0, 1)]).astype(np.int32)
        seg_w = np.stack([np.searchsorted(tw[s][0], np.arange(w + 1)) for s in (0, 1)]).astype(np.int32)
        n = b * hu * wu
        _, r, wgt = _virtual_tables(b, h, w, hu, wu, dev, torch.float32)
        rhs = torch.zeros((4, 4 * n), dtype=torch.float32, device=dev)
        rhs[0] = r[..., 0].reshape(-1)
        rhs[1] = r[..., 1].reshape(-1)
        rhs[2] = 1.0
        return {"seg_h": torch.from_numpy(seg_h).to(dev), "seg_w": torch.from_numpy(seg_w).to(dev),
                "wgt": wgt.contiguous(), "rhs_t": T.tile_planes(rhs), "cell": (cell_h, cell_w)}
    return T.lru(_geo_cache, (b, h, w, hu, wu, str(dev)), build)


def cell_sum(g1: torch.Tensor, b: int, h: int, w: int, hu: int, wu: int,
             dp: Optional[torch.Tensor] = None, dp_t: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``diinn_liif_cell_sum`` on g_a,1 (tiled over the virtual pixels, [ceil(4 N / 32), 256, 32]): (dP1 in planes 0..255 of an NCHW
    [B,1024,H,W] buffer, the same in rows 0..255 of a tiled [ceil(B H W / 32), 1024, 32] group).  Given buffers are written in place."""
    dev = g1.device
    cells = b * h * w
    tc = (cells + PLANE_TILE - 1) // PLANE_TILE
    geo = _geometry(b, h, w, hu, wu, dev)
    if dp is None:
        dp = torch.empty((b, 4 * HIDDEN, h, w), dtype=torch.float32, device=dev)
    if dp_t is None:                                             # (a ragged last tile's padding stays zero)
        dp_t = (torch.empty if cells % PLANE_TILE == 0 else torch.zeros)((tc, 4 * HIDDEN, PLANE_TILE), dtype=torch.float32, device=dev)
    with _native.launcher(dev) as run:
        run("diinn_liif_cell_sum", g1, geo["seg_h"], geo["seg_w"], dp, dp_t, b, h, w, hu, wu)
    return dp, dp_t


def backward_fused(gout: torch.Tensor, feat: torch.Tensor, acts: torch.Tensor, image: torch.Tensor, w0: torch.Tensor, wkey, wpins,
                   size: Sequence[int], need_feat_grad: bool = True, need_w0_grad: bool = True, split: Optional[torch.Tensor] = None
                   ) -> Tuple[Optional[torch.Tensor], List[Optional[torch.Tensor]]]:
    """The same gradients as ``liif_backward_reference``, on the HIP kernels throughout (module docstring).  ``acts``: the tiled
    buffer of ``train_forward``; ``w0``: imnet.layers.0.weight; ``wkey`` / ``wpins`` identify its values for the cache of the
    transposed conv weight.  ``need_w0_grad`` false skips the conv's weight GEMM (d layers.0.weight is then None).
    ``split`` (the split training image of ``image``, ``liif_split_training.split_on_device``): the chain runs on
    ``diinn_liif_backward_data_x3`` -- the three transposed products in split-bf16 arithmetic -- and nothing else differs."""
    b, _, h, w = feat.shape
    hu, wu = int(size[0]), int(size[1])
    n = b * hu * wu
    vn = 4 * n
    t = virtual_tiles(n)
    dev = gout.device
    if tuple(acts.shape) != (4, t, HIDDEN, PLANE_TILE) or not acts.is_contiguous():
        raise ValueError("acts must be the contiguous tiled [4, T, 256, 32] buffer of the training forward")
    geo = _geometry(b, h, w, hu, wu, dev)
    cell_h, cell_w = geo["cell"]
    gp = gout.to(torch.float32).permute(1, 0, 2, 3).reshape(3, n).contiguous()
    g = torch.empty((4, t, HIDDEN, PLANE_TILE), dtype=torch.float32, device=dev)
    # the head product's right-hand side: rows w_v g_0, w_v g_1, w_v g_2, 0 over the virtual pixels
    wg = (geo["wgt"].view(1, 4, n) * gp.view(3, 1, n)).reshape(3, vn)
    wg_t = T.tile_planes(torch.cat([wg, wg.new_zeros((1, vn))], 0))
    ksplit = max(1, min(2 * T.WGRAD_KSPLIT, t))                   # 256 rows = 2 output blocks: twice mode 3's splits fill the CUs
    rsplit = max(1, min(T.ROWDOT_SPLITS, t))
    part = torch.empty((3, ksplit, HIDDEN, HIDDEN + 1), dtype=torch.float32, device=dev)
    part1 = torch.empty((rsplit, HIDDEN, 4), dtype=torch.float32, device=dev)
    partl = torch.empty((rsplit, HIDDEN, 4), dtype=torch.float32, device=dev)
    with _native.launcher(dev) as run:
        if split is None:
            run("diinn_liif_backward_data", gp, acts, image, g, b, h, w, hu, wu)
        else:
            run("diinn_liif_backward_data_x3", gp, acts, image, split, g, b, h, w, hu, wu)
        for li in (3, 2, 1):                                      # [dW_l | db_l] = g_a,l . h_{l-1}^T, l = li + 1
            run("diinn_plane_gemm_nt", g[li], HIDDEN, 0, acts[li - 1], HIDDEN, 0, part[li - 1], HIDDEN, HIDDEN, vn, ksplit, 1)
        run("diinn_plane_rowdot", acts[3], HIDDEN, wg_t, partl, HIDDEN, vn, rsplit)
        run("diinn_plane_rowdot", g[0], HIDDEN, geo["rhs_t"], part1, HIDDEN, vn, rsplit)
    dp, dp_t = cell_sum(g[0], b, h, w, hu, wu)
    dl = T._sum_parts(partl.view(1, rsplit, -1)).view(HIDDEN, 4)      # [256, 4]: h_4 . (w_v g ; 0)^T
    dws = T._sum_parts(part.view(3, ksplit, -1)).view(3, HIDDEN, HIDDEN + 1)
    d1 = T._sum_parts(part1.view(1, rsplit, -1)).view(HIDDEN, 4)      # [256, 4]: g_a,1 . (rel_h, rel_w, 1, 0)^T
    wx = lambda: w0.detach()[:, :UNFOLD].reshape(HIDDEN, T.IN_CHANNELS, 3, 3).contiguous()      # noqa: E731
    d_wx, d_feat = T._conv_grads_native(feat, wx, dp, need_feat_grad, want_weight=need_w0_grad, wkey=wkey, wpins=wpins, a_t=dp_t, rows=HIDDEN)
    d_w0 = None
    if need_w0_grad:
        d_w0 = torch.cat([d_wx, d1[:, :2], d1[:, 2:3] * cell_h, d1[:, 2:3] * cell_w], dim=1)
    grads: List[Optional[torch.Tensor]] = [d_w0, d1[:, 2].contiguous()]
    for li in (1, 2, 3):
        grads += [dws[li - 1][:, :HIDDEN].contiguous(), dws[li - 1][:, HIDDEN].contiguous()]
    grads += [dl[:, :3].t().contiguous(), gp.sum(1)]
    return d_feat, grads


class LIIFFunction(torch.autograd.Function):
    """out = LIIF decoder(feat) on the HIP kernels, differentiable in feat and the ten imnet tensors (PARAM_NAMES order)."""

    @staticmethod
    def forward(ctx, feat: torch.Tensor, hu: int, wu: int, *params: torch.Tensor) -> torch.Tensor:
        feat_c = T.checked_features(feat, params, PARAM_NAMES, PARAM_SHAPES, 4 * hu, wu, HIDDEN)     # the limit counts virtual pixels
        image = image_on_device(params)
        out, acts = train_forward(feat_c, image, hu, wu)
        ctx.save_for_backward(feat_c, acts, image, params[0].detach())
        ctx.size = (hu, wu)
        ctx.wkey = ("liif", params[0].data_ptr(), params[0]._version)
        ctx.wpins = (params[0],)
        return out

    @staticmethod
    def backward(ctx, gout: torch.Tensor):
        feat, acts, image, w0 = ctx.saved_tensors
        need = ctx.needs_input_grad
        d_feat, d_params = backward_fused(gout, feat, acts, image, w0, ctx.wkey, ctx.wpins, ctx.size,
                                          need_feat_grad=need[0], need_w0_grad=need[3])
        return T.function_grads(ctx, d_feat, d_params, 3)


def decode_with_grad(imnet, feat: torch.Tensor, size: Sequence[int]) -> torch.Tensor:
    """``LIIF.query_rgb`` + ``reshape_pred`` of every HR pixel under autograd; ``imnet`` is the model's MLP (modules.MLP)."""
    hu, wu = size
    return LIIFFunction.apply(feat, int(hu), int(wu), *T.named_params(imnet, PARAM_NAMES))
