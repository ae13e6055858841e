"""Training path of the decoder with ``init_q=True``, mode 3: autograd through the HIP kernels.  Opt-in: ``ImplicitDecoder.hip_autograd``.

The reference trains by ``ImplicitDecoder.forward(x, size, None)`` under autograd (sr_module.py:127-129 -> diinn.py:170-171 -> step(),
:132-139, with the per-pixel sine embedding of :48-51,113-115).  Per HR pixel, with syn = (rel_h, rel_w, ratio), X the 576 unfolded
features of the pixel's LR cell (zero outside the map), Wx_0 = K.0.weight, Wx_i = K.i.weight[:, 256:], Wq_i = K.i.weight[:, :256]::

    a   = Fw syn + bF            E = sin(a)            x' = E * X
    k_0 = relu(Wx_0 x' + bK_0)                         s_0 = Q0 E + bQ0             q_0 = k_0 sin(s_0)
    k_i = relu(Wq_i q_{i-1} + Wx_i x' + bK_i)          s_i = Qw_i q_{i-1} + bQ_i    q_i = k_i sin(s_i)       out = L q_3 + bL

  forward   initq_planes_kernel in its radians form (the planes of the WHOLE image, 5,120 bytes per HR pixel), then
            decode_kernel<SIN | DECODE_INITQ, true, SAVE> (C ABI ``diinn_decode_initq_train_fwd``): every layer's k_i and s_i as
            tiled planes, in ``diinn_decode_train_fwd``'s layout.
  backward  ``backward_fused_initq``: the per-pixel chain is mode 3's, unchanged (``diinn_backward_data``: G_i = (g_a,i ; g_s,i) and
            q_i; the plane GEMMs of d[Wq_i ; Qw_i], the head's rowdot).  New: initq_bwd_kernel (``diinn_initq_backward``) takes
            dx' = sum_i Wx_i^T g_a,i and Q0^T g_s,0 on the fp32 MFMA and writes U = dx' * E, da = (dx' * X + Q0^T g_s,0) * cos a,
            x' and E as tiled groups; dWx_i^T = x' . g_a,i^T and dQ0^T = E . g_s,0^T are the library's plane GEMM, (dFw | dbF) its
            rowdot of da against (rel_h, rel_w, ratio, 1); the features' gradient is the per-cell sum of U (cell_sum_rows_kernel)
            folded (fold3x3_kernel, the adjoint of unfold3x3).  No framework convolution, GEMM or F.fold.
            ``backward_from_saved_initq`` states the same gradients in device-agnostic tensor algebra: the unit-tested formula
            sheet (CPU, against the reference's own .grad fixtures) and the on-GPU cross-check of the fused path.

Two weight images travel with a step, both rebuilt on the device by one gather each after an optimiser step: the body image (mode 3's
training image of the K / Q.1..3 / head tensors with a zero Q0 table; no Winograd section: there is no hoisted conv) and the init_q
TRAINING image (``pack_initq_train``: the init_q image's layout in radians -- a pure permutation, so the division by 2 pi of the
inference image never has to be redone on the device -- followed by Wx^T and Q0^T as initq_bwd_kernel's MFMA A operands).
"""
from __future__ import annotations

import functools
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _native
from .training import (HIDDEN, IN_CHANNELS, PARAM_NAMES, PARAM_SHAPES, PLANE_TILE, UNFOLD, ChainStage, _cell_sum, _sum_parts,
                       checked_features, coordinate_tensors, function_grads, gather_index, index_on, kept, named_params,
                       pack_gather_index, position_state_dict, train_buffers, weights_key)

PAD_ROWS = 640             # the 576 unfolded rows padded to 5 x 128: diinn_plane_gemm_nt wants M % 128 == 0
WGRAD_X_KSPLIT = 51        # pixel-axis splits of the x' / E weight-gradient GEMMs: 5 output blocks x 51 = 255 workgroups, one per CU

# the reference's registration order with init_q (ImplicitDecoder.__init__, diinn.py:48-51 first, then :73-80,92)
INITQ_PARAM_NAMES: List[str] = ["first_layer.0.weight", "first_layer.0.bias"] + PARAM_NAMES
INITQ_PARAM_SHAPES: Dict[str, Tuple[int, ...]] = {
    **PARAM_SHAPES, "first_layer.0.weight": (UNFOLD, 3, 1, 1), "first_layer.0.bias": (UNFOLD,),
    "Q.0.0.weight": (HIDDEN, UNFOLD, 1, 1),
}
# the tensors the training image is built from, in the order of its gather's flat vector
IMAGE_NAMES: List[str] = ["first_layer.0.weight", "first_layer.0.bias", "Q.0.0.weight", "Q.0.0.bias"] + [f"K.{i}.0.weight" for i in range(4)]


def pack_initq_train(sd, prefix: str = "") -> torch.Tensor:
    """The init_q TRAINING image (1-D fp32 CPU tensor; C ABI ``diinn_pack_initq_train``, layout in include/diinn_hip.h) of the
    reference-named tensors ``first_layer.0.*``, ``Q.0.0.*`` and ``K.0..3.0.weight`` in ``sd``."""
    from .decoder import _host_array
    lib = _native.load()
    fw, fb = _host_array(sd, prefix, "first_layer.0.weight", (UNFOLD, 3)), _host_array(sd, prefix, "first_layer.0.bias", (UNFOLD,))
    q0w, q0b = _host_array(sd, prefix, "Q.0.0.weight", (HIDDEN, UNFOLD)), _host_array(sd, prefix, "Q.0.0.bias", (HIDDEN,))
    k0w = _host_array(sd, prefix, "K.0.0.weight", (HIDDEN, UNFOLD))
    kw = [_host_array(sd, prefix, f"K.{i}.0.weight", (HIDDEN, HIDDEN + UNFOLD)) for i in (1, 2, 3)]
    packed = np.empty(lib.diinn_initq_train_packed_floats(), dtype=np.float32)
    _native.check(lib.diinn_pack_initq_train(_native.fptr(fw), _native.fptr(fb), _native.fptr(q0w), _native.fptr(q0b), _native.fptr(k0w),
                                             _native._f3(*[_native.fptr(a) for a in kw]), _native.fptr(packed)), "diinn_pack_initq_train")
    return torch.from_numpy(packed)


def image_word() -> int:
    """Float index of the training image's validity word (behind BQ0, where the init_q image keeps its own)."""
    return UNFOLD * 4 + 8 * (UNFOLD // 8) * 256 + HIDDEN


@functools.lru_cache(maxsize=None)
def train_image_gather_index() -> torch.Tensor:
    """int64 [image floats]: image[i] = flat[index[i]] with ``flat`` the IMAGE_NAMES tensors flattened in order followed by one 0.0
    (the padding rows and the validity word point at it; the word is written after the gather).  Derived by packing a state dict
    whose values are their own flat position (exact in fp32), as ``training.pack_gather_index``."""
    sd, total = position_state_dict(IMAGE_NAMES, INITQ_PARAM_SHAPES)
    packed = pack_initq_train(sd).numpy()
    word = image_word()
    if packed[word:word + 1].view(np.uint32)[0] != _native.INITQ_TRAIN_MAGIC:
        raise RuntimeError("the init_q training image carries no validity word where the layout says")
    # (the q-columns of K.1..3 -- Wq_i -- live in the body image, not here)
    need = np.ones(total, bool)
    off = 0
    for name in IMAGE_NAMES:
        n = int(np.prod(INITQ_PARAM_SHAPES[name]))
        if name in ("K.1.0.weight", "K.2.0.weight", "K.3.0.weight"):
            need[off:off + n].reshape(HIDDEN, HIDDEN + UNFOLD)[:, :HIDDEN] = False
        off += n
    return gather_index(packed, total, [(word, 1)], "the init_q training image", need=need)


def pack_train_image_on_device(p: Dict[str, torch.Tensor]) -> torch.Tensor:
    """``pack_initq_train`` of the named tensors ``p`` on their GPU: one gather and the validity word."""
    dev = p["Q.0.0.weight"].device
    flat = torch.cat([p[name].detach().reshape(-1).to(torch.float32) for name in IMAGE_NAMES] + [torch.zeros(1, device=dev)])
    image = flat.index_select(0, index_on(dev, "initq", train_image_gather_index))
    word = image_word()
    image[word:word + 1].view(torch.int32).fill_(_native.INITQ_TRAIN_MAGIC)
    return image


def pack_body_on_device(p: Dict[str, torch.Tensor]) -> torch.Tensor:
    """The body image on the GPU: mode 3's gathered training image (permutation sections only; the inference entry points answer
    NaN on it) of the K / Q.1..3 / head tensors with a zero [256,3] in place of the 576-wide ``Q.0.0.weight``, whose rows the init_q
    kernels never read.  No Winograd section: this configuration has no hoisted conv."""
    dev = p["Q.0.0.weight"].device
    parts = [torch.zeros(HIDDEN * 3, device=dev) if name == "Q.0.0.weight" else p[name].detach().reshape(-1).to(torch.float32)
             for name in PARAM_NAMES]
    return torch.cat(parts + [torch.zeros(1, device=dev)]).index_select(0, index_on(dev, 3, pack_gather_index))


def images_on_device(params: Sequence[torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
    """(body image, init_q training image) of the INITQ_PARAM_NAMES tensors on their GPU.  The last pair is kept while no parameter has
    been modified (a training step decodes once per scale with the same weights); the entry pins the tensors its key describes."""
    def build():
        p = dict(zip(INITQ_PARAM_NAMES, params))
        return pack_body_on_device(p), pack_train_image_on_device(p)
    return kept("initq", weights_key(params), params, build)


# ---------------------------------------------------------------------------
# backward from the saved planes (device-agnostic tensor algebra)
# ---------------------------------------------------------------------------
def embedding_planes(feat: torch.Tensor, p: Dict[str, torch.Tensor], size: Sequence[int]):
    """(a [576, Hu*Wu], X [576, N], syn [3, Hu*Wu]) in ``feat``'s dtype: the first layer's sine argument per HR pixel (it does not depend
    on the batch item), the unfolded features of every pixel's LR cell (pixel index (b*Hu + y)*Wu + x), the synthesis input."""
    b, c, h, w = feat.shape
    hu, wu = int(size[0]), int(size[1])
    dev, dt = feat.device, feat.dtype
    idx_h, rel_h, idx_w, rel_w, ratio = coordinate_tensors(h, w, hu, wu, dev)
    syn = torch.empty((3, hu, wu), dtype=dt, device=dev)
    syn[0] = rel_h.to(dt)[:, None]
    syn[1] = rel_w.to(dt)[None, :]
    syn[2] = ratio
    syn = syn.reshape(3, hu * wu)
    a = p["first_layer.0.weight"].reshape(UNFOLD, 3).to(dt) @ syn + p["first_layer.0.bias"].reshape(UNFOLD, 1).to(dt)
    unf = torch.nn.functional.unfold(feat, 3, padding=1).view(b, c * 9, h, w)
    xc = unf[:, :, idx_h][:, :, :, idx_w].permute(1, 0, 2, 3).reshape(c * 9, b * hu * wu)
    return a, xc, syn


def backward_from_saved_initq(gout: torch.Tensor, feat: torch.Tensor, acts: torch.Tensor, params: Sequence[torch.Tensor],
                              size: Sequence[int], need_feat_grad: bool = True, product=None
                              ) -> Tuple[Optional[torch.Tensor], List[torch.Tensor]]:
    """Gradients of the ``init_q=True``, mode-3 decoder given d(loss)/d(out): the formula sheet (any device, the dtype of ``acts``).
    ``product(w_t, g)``: how the four transposed per-pixel products -- the chain's Wq_i^T g_a,i and Qw_i^T g_s,i, dx' 's Wx_i^T g_a,i
    and t = Q0^T g_s,0 -- are formed; None: a plain matmul (``initq_split_training`` passes the split-bf16 product).

    gout [B,3,Hu,Wu]; feat [B,64,H,W]; acts [4,2,256,N] plain planes k_i, s_i (radians); params in INITQ_PARAM_NAMES order.
    Returns (d feat or None, [d param ...] in INITQ_PARAM_NAMES order).  With the gates of mode 3,
        g_a,i = g_q,i * sin(s_i) * [k_i > 0]        g_s,i = g_q,i * k_i * cos(s_i)        g_q,i-1 = Wq_i^T g_a,i + Qw_i^T g_s,i,
    per pixel   dx' = sum_i Wx_i^T g_a,i      dE = dx' * X + Q0^T g_s,0      U = dx' * E      da = dE * cos(a)
    and summed over the pixels
        dWx_i = g_a,i x'^T     dbK_i = rowsum g_a,i     dQ0 = g_s,0 E^T     dbQ0 = rowsum g_s,0     dFw = da syn^T     dbF = rowsum da
        dfeat = fold3x3(per-cell sums of U)   (the adjoint of unfold3x3; the features get no other gradient)."""
    dt = acts.dtype
    if product is None:
        product = torch.matmul
    p = {name: t.to(dt) for name, t in zip(INITQ_PARAM_NAMES, params)}
    feat = feat.to(dt)
    b, _, h, w = feat.shape
    hu, wu = int(size[0]), int(size[1])
    n = b * hu * wu
    dev = gout.device
    idx_h, _, idx_w, _, _ = coordinate_tensors(h, w, hu, wu, dev)
    a, xc, syn = embedding_planes(feat, p, size)
    e = torch.sin(a).repeat(1, b)                                  # [576, N]: the same for every batch item
    cos_a = torch.cos(a).repeat(1, b)
    syn_n = syn.repeat(1, b)
    xp = e * xc
    grads: Dict[str, torch.Tensor] = {}

    g_out = gout.to(dt).permute(1, 0, 2, 3).reshape(3, n)
    q3 = acts[3, 0] * torch.sin(acts[3, 1])
    grads["last_layer.weight"] = (g_out @ q3.t()).reshape(3, HIDDEN, 1, 1)
    grads["last_layer.bias"] = g_out.sum(1)
    g_q = p["last_layer.weight"].reshape(3, HIDDEN).t() @ g_out
    dxp = torch.zeros_like(xp)
    for i in (3, 2, 1, 0):
        k, s = acts[i, 0], acts[i, 1]
        g_a = g_q * torch.sin(s) * (k > 0)
        g_s = g_q * k * torch.cos(s)
        wfull = p[f"K.{i}.0.weight"].reshape(HIDDEN, -1)
        wx = wfull[:, HIDDEN:] if i else wfull
        dxp += product(wx.t(), g_a)
        d_wx = g_a @ xp.t()
        grads[f"K.{i}.0.bias"] = g_a.sum(1)
        grads[f"Q.{i}.0.bias"] = g_s.sum(1)
        if i:
            q_prev = acts[i - 1, 0] * torch.sin(acts[i - 1, 1])
            grads[f"K.{i}.0.weight"] = torch.cat([g_a @ q_prev.t(), d_wx], 1).reshape(HIDDEN, HIDDEN + UNFOLD, 1, 1)
            grads[f"Q.{i}.0.weight"] = (g_s @ q_prev.t()).reshape(HIDDEN, HIDDEN, 1, 1)
            g_q = product(wfull[:, :HIDDEN].t(), g_a) + product(p[f"Q.{i}.0.weight"].reshape(HIDDEN, HIDDEN).t(), g_s)
        else:
            grads["K.0.0.weight"] = d_wx.reshape(HIDDEN, UNFOLD, 1, 1)
            grads["Q.0.0.weight"] = (g_s @ e.t()).reshape(HIDDEN, UNFOLD, 1, 1)
            d_e = dxp * xc + product(p["Q.0.0.weight"].reshape(HIDDEN, UNFOLD).t(), g_s)
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
def backward_fused_initq(gout: torch.Tensor, feat: torch.Tensor, acts: torch.Tensor, packed: torch.Tensor, image: torch.Tensor,
                         size: Sequence[int], need_feat_grad: bool = True, qonly: bool = False,
                         head: Optional[torch.Tensor] = None, split: Optional[torch.Tensor] = None,
                         initq_split: Optional[torch.Tensor] = None) -> Tuple[Optional[torch.Tensor], List[torch.Tensor]]:
    """The same gradients as ``backward_from_saved_initq``, on the HIP kernels throughout:
      diinn_backward_data     3 x bwd_layer_kernel: the per-pixel chain of mode 3, unchanged; leaves G_i = (g_a,i ; g_s,i) and q_i
      diinn_plane_gemm_nt     [dWq_i ; dQw_i | bias sums] = G_i . q_{i-1}^T (i = 1..3), as in mode 3
      diinn_plane_rowdot      G_0 against (rel_h, rel_w, ratio, 1): column 3 is (dbK_0 ; dbQ0); the head against g_out
      diinn_initq_backward    initq_bwd_kernel: U, da, x', E as tiled groups (9,728 bytes per HR pixel)
      diinn_plane_gemm_nt     dWx_i^T [640 x 256] = x' . g_a,i^T (i = 0..3) and dQ0^T = E . g_s,0^T
      diinn_plane_rowdot      (dFw | dbF) = da . (rel_h, rel_w, ratio, 1)^T
      diinn_cell_sum_rows, diinn_fold3x3    dfeat = fold3x3(per-cell sums of U)
    ``acts`` is the tiled buffer [4, T, 512, 32] of the training forward, ``packed`` / ``image`` the two images it ran on.

    The other decoder modes with ``init_q`` (initq_modes_training.py) change the CHAIN -- the first two lines above -- and nothing behind it:
      ``qonly`` (modes 1/2, K.1..3 in mode 2's shape)  diinn_backward_data_qonly, then diinn_pixel_chain_bwd completes g_a,i in place over
                rows 0..255 of G_i; [dKk_i | dbK_i] = g_a,i . k_{i-1}^T (rows 0..255 of ``acts[i-1]``) and [dQw_i | dbQ_i] = g_s,i . q_{i-1}^T
                are two 256-row plane GEMMs per layer in place of the stacked 512-row one;
      ``head``  (mode 4: the 3x3 head image; ``packed`` is the body image with a zero 1x1 head)  diinn_backward_data_head3x3, and
                d last_layer.weight [3,256,3,3] from q_3 against the seven 4-row groups of dT, as in ``training.backward_fused``.
    Mode 3 in split-bf16 arithmetic (initq_split_training.py) exchanges two kernels, each by a keyword of its own, so that the fp32 and
    the split forms mix:
      ``split``        the split training image of ``packed``: the chain on diinn_backward_data_x3 (bwd_layer_x3_kernel);
      ``initq_split``  the init_q split training image: diinn_initq_backward_x3 (initq_bwd_x3_kernel) in place of diinn_initq_backward."""
    c = ChainStage(gout, feat, acts, packed, size, head=head, qonly=qonly, split=split)
    b, h, w, hu, wu, n, t, g = c.b, c.h, c.w, c.hu, c.wu, c.n, c.t, c.g
    syn_t = c.geo["syn_t"]
    f32 = dict(dtype=torch.float32, device=c.dev)
    u_t = torch.empty((t, UNFOLD, PLANE_TILE), **f32)
    da_t = torch.empty((t, UNFOLD, PLANE_TILE), **f32)
    xp_t = torch.empty((t, PAD_ROWS, PLANE_TILE), **f32)
    e_t = torch.empty((t, PAD_ROWS, PLANE_TILE), **f32)
    xsplit = max(1, min(WGRAD_X_KSPLIT, t))
    rsplit = c.rsplit
    partx = torch.empty((5, xsplit, PAD_ROWS, HIDDEN), **f32)
    partf = torch.empty((rsplit, 2 * HIDDEN, 4), **f32)           # (dFw | dbF): the rowdot takes at most 512 rows per launch --
    partg = torch.empty((rsplit, UNFOLD - 2 * HIDDEN, 4), **f32)   # rows 0..511, then rows 512..575
    d_feat = None
    with _native.launcher(c.dev) as run:
        c.launch(run)
        if initq_split is None:
            run("diinn_initq_backward", feat, g, image, u_t, da_t, xp_t, e_t, b, h, w, hu, wu)
        else:
            run("diinn_initq_backward_x3", feat, g, image, initq_split, u_t, da_t, xp_t, e_t, b, h, w, hu, wu)
        for i in range(4):                                       # dWx_i^T [640 x 256] = x' . g_a,i^T
            run("diinn_plane_gemm_nt", xp_t, PAD_ROWS, 0, g[i], 2 * HIDDEN, 0, partx[i], PAD_ROWS, HIDDEN, n, xsplit, 0)
        run("diinn_plane_gemm_nt", e_t, PAD_ROWS, 0, g[0], 2 * HIDDEN, HIDDEN, partx[4], PAD_ROWS, HIDDEN, n, xsplit, 0)
        run("diinn_plane_rowdot", da_t, UNFOLD, syn_t, partf, 2 * HIDDEN, n, rsplit)
        run("diinn_plane_rowdot", (da_t, 2 * HIDDEN * PLANE_TILE), UNFOLD, syn_t, partg, UNFOLD - 2 * HIDDEN, n, rsplit)
        if need_feat_grad:
            d_unf = torch.empty((b, UNFOLD, h, w), **f32)
            d_feat = torch.empty((b, IN_CHANNELS, h, w), **f32)
            run("diinn_cell_sum_rows", u_t, UNFOLD, UNFOLD, c.geo["seg_h"], c.geo["seg_w"], d_unf, b, h, w, hu, wu)
            run("diinn_fold3x3", d_unf, d_feat, b, IN_CHANNELS, h, w)
    grads: Dict[str, torch.Tensor] = {}
    d_wq, d_bk = c.grads(grads)
    dxs = _sum_parts(partx.view(5, xsplit, -1)).view(5, PAD_ROWS, HIDDEN)[:, :UNFOLD].transpose(1, 2)   # [5, 256, 576]: dWx_0..3, dQ0
    d0 = c.layer0()
    df = torch.cat([_sum_parts(partf.view(1, rsplit, -1)).view(2 * HIDDEN, 4),
                    _sum_parts(partg.view(1, rsplit, -1)).view(UNFOLD - 2 * HIDDEN, 4)], 0)               # [576, 4]: (dFw | dbF)
    grads["first_layer.0.weight"] = df[:, :3].reshape(UNFOLD, 3, 1, 1)
    grads["first_layer.0.bias"] = df[:, 3]
    grads["K.0.0.weight"] = dxs[0].reshape(HIDDEN, UNFOLD, 1, 1)
    grads["K.0.0.bias"] = d0[:HIDDEN, 3]
    grads["Q.0.0.weight"] = dxs[4].reshape(HIDDEN, UNFOLD, 1, 1)
    grads["Q.0.0.bias"] = d0[HIDDEN:, 3]
    for i in (3, 2, 1):
        grads[f"K.{i}.0.weight"] = torch.cat([d_wq[i], dxs[i]], dim=1).reshape(HIDDEN, HIDDEN + UNFOLD, 1, 1)
        grads[f"K.{i}.0.bias"] = d_bk[i]
    return d_feat, [grads[name] for name in INITQ_PARAM_NAMES]


def train_forward_initq(feat_c: torch.Tensor, params: Sequence[torch.Tensor], hu: int, wu: int, sin_mode: int):
    """The training forward on a contiguous fp32 CUDA ``feat_c``.  Returns (out, acts [4,T,512,32], body image, training image)."""
    b, _, h, w = feat_c.shape
    packed, image = images_on_device(params)
    acts, out, pix = train_buffers(feat_c, hu, wu, _native.load().diinn_initq_pix_bytes(b, wu, hu) // 4)
    with _native.launcher(feat_c.device) as run:
        run("diinn_decode_initq_train_fwd", feat_c, packed, image, pix, out, acts, b, h, w, hu, wu, int(sin_mode))
    return out, acts, packed, image


class DecodeInitqFunction(torch.autograd.Function):
    """out = decoder(feat) for ``init_q=True``, mode 3, on the HIP kernels: differentiable in feat and the 20 parameter tensors
    (INITQ_PARAM_NAMES order).  The pixel planes (5,120 bytes per HR pixel) are dropped after the forward; the backward needs the
    saved k_i / s_i planes, the features and the two images."""

    @staticmethod
    def forward(ctx, feat: torch.Tensor, hu: int, wu: int, sin_mode: int, *params: torch.Tensor) -> torch.Tensor:
        feat_c = checked_features(feat, params, INITQ_PARAM_NAMES, INITQ_PARAM_SHAPES, hu, wu, PAD_ROWS, " for decoder mode 3 with init_q")
        out, acts, packed, image = train_forward_initq(feat_c, params, hu, wu, sin_mode)
        ctx.save_for_backward(feat_c, acts, packed, image)
        ctx.size = (hu, wu)
        return out

    @staticmethod
    def backward(ctx, gout: torch.Tensor):
        feat, acts, packed, image = ctx.saved_tensors
        d_feat, d_params = backward_fused_initq(gout.contiguous(), feat, acts, packed, image, ctx.size,
                                                need_feat_grad=ctx.needs_input_grad[0])
        return function_grads(ctx, d_feat, d_params, 4)


def decode_with_grad(decoder, feat: torch.Tensor, size: Sequence[int]) -> torch.Tensor:
    """``ImplicitDecoder(mode=3, init_q=True, hip_autograd=True).forward(x, size, None)`` under autograd."""
    hu, wu = size
    return DecodeInitqFunction.apply(feat, int(hu), int(wu), int(decoder.sin_mode), *named_params(decoder, INITQ_PARAM_NAMES))
