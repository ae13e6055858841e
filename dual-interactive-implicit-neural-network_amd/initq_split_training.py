"""``init_q=True``, mode 3, under autograd in split-bf16 arithmetic -- the opt-in ``ImplicitDecoder.hip_autograd_initq_split_bf16``
together with ``hip_initq_split_bf16`` and ``compute="bf16x3"``.

The step of ``initq_training.DecodeInitqFunction`` with every fp32-MFMA kernel exchanged for its split-bf16 form -- a product is
``w_lo.x_hi + w_hi.x_lo + w_hi.x_hi`` on v_mfma_f32_32x32x16_bf16 with fp32 accumulation; hi = bf16(v), lo = bf16(v - hi) -- and two
images added:

  images    the SPLIT TRAINING image of the body image (``diinn_pack_split_train`` on ``initq_training.pack_body_on_device``'s image:
            the layers and their transposes, as for mode 3) and the INIT_Q SPLIT TRAINING image (csrc/diinn_layout.h;
            ``diinn_pack_initq_split_train``: Wx and Q0 in the planes kernel's piece order, Wx^T and Q0^T in the backward kernel's,
            all in radians).  Both are filled on the device once per weight version and cached under ``training.kept``.
  forward   ``diinn_decode_initq_train_fwd_x3``: initq_planes_x3_kernel<SIN | INITQ_X3_RAD>, then
            decode_bf16x3_kernel<SIN | X3_INITQ | X3_SAVE>.  The same fp32 planes k_i, s_i (radians) as the fp32 forward.
  backward  ``initq_training.backward_fused_initq(..., split=, initq_split=)``: the chain on 3 x bwd_layer_x3_kernel
            (``diinn_backward_data_x3``) and initq_bwd_x3_kernel (``diinn_initq_backward_x3``) in place of initq_bwd_kernel.  The plane
            GEMMs, the rowdots, the cell sum and the fold are unchanged and fp32.

Because the planes keep the fp32 contract, the two forwards and the two forms of either backward kernel mix: each is chosen by a
keyword of its own (the tests' bisecting tool).

The EMULATION SHEET (``split_forward_reference``, ``split_backward_reference``) states the same arithmetic in torch fp32 on any
device.  What an end-to-end gradient comparison cannot hold is the ReLU kink: here ``k_0`` comes from a split GEMM
too, so all four layers' gates can flip."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _native
from . import initq_training as IT
from . import sheets as S
from . import training as T
from .initq_training import INITQ_PARAM_NAMES, INITQ_PARAM_SHAPES, PAD_ROWS
from .sheets import split_hi_lo, split_matmul
from .training import HIDDEN, UNFOLD


# ---------------------------------------------------------------------------
# the images
# ---------------------------------------------------------------------------
def initq_split_train_floats() -> int:
    return int(_native.load().diinn_initq_split_train_floats())


def image_word() -> int:
    """Float index of the init_q split training image's validity word (behind Q0X)."""
    return (16 + 4) * 4 * 9 * 2 * 2 * 256


def pack_initq_split_host(body: np.ndarray, train_image: np.ndarray) -> np.ndarray:
    """Host twin of the device packer: a host body image holding section WP (``decoder.pack_state_dict(initq_body_state_dict(sd))``)
    and the host init_q training image (``initq_training.pack_initq_train(sd)``) -> the init_q split training image, float32
    [1,556,484] whose bytes are the bf16 pieces."""
    body = np.ascontiguousarray(body, dtype=np.float32)
    train_image = np.ascontiguousarray(train_image, dtype=np.float32)
    out = np.empty(initq_split_train_floats(), dtype=np.float32)
    _native.check(_native.load().diinn_pack_initq_split_train_host(_native.fptr(body), _native.fptr(train_image), _native.fptr(out)),
                  "diinn_pack_initq_split_train_host")
    return out


def split_images_on_device(params: Sequence[torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
    """(split training image of the body image, init_q split training image) of the INITQ_PARAM_NAMES tensors on their GPU, from
    ``initq_training.images_on_device``'s pair.  Kept, like that pair, while no parameter has been modified."""
    def build():
        packed, image = IT.images_on_device(params)
        split = torch.empty(int(_native.load().diinn_split_train_floats()), dtype=torch.float32, device=packed.device)
        initq_split = torch.empty(initq_split_train_floats(), dtype=torch.float32, device=packed.device)
        with _native.launcher(packed.device) as run:
            run("diinn_pack_split_train", packed, split)
            run("diinn_pack_initq_split_train", packed, image, initq_split)
        return split, initq_split
    return T.kept("initq_split", T.weights_key(params), params, build)


# ---------------------------------------------------------------------------
# forward and the autograd function
# ---------------------------------------------------------------------------
def train_forward_initq_split(feat_c: torch.Tensor, params: Sequence[torch.Tensor], hu: int, wu: int, sin_mode: int):
    """The split training forward on a contiguous fp32 CUDA ``feat_c``.  Returns (out, acts [4,T,512,32], body image, init_q training
    image, split training image, init_q split training image)."""
    b, _, h, w = feat_c.shape
    packed, image = IT.images_on_device(params)
    split, initq_split = split_images_on_device(params)
    acts, out, pix = T.train_buffers(feat_c, hu, wu, _native.load().diinn_initq_pix_bytes(b, wu, hu) // 4)
    with _native.launcher(feat_c.device) as run:
        run("diinn_decode_initq_train_fwd_x3", feat_c, packed, image, split, initq_split, pix, out, acts, b, h, w, hu, wu, int(sin_mode))
    return out, acts, packed, image, split, initq_split


class DecodeInitqSplitFunction(torch.autograd.Function):
    """out = decoder(feat) for ``init_q=True``, mode 3, in split-bf16 arithmetic both ways, differentiable in feat and the 20 parameter
    tensors (INITQ_PARAM_NAMES order): ``initq_training.DecodeInitqFunction`` on diinn_decode_initq_train_fwd_x3 /
    diinn_backward_data_x3 / diinn_initq_backward_x3."""

    @staticmethod
    def forward(ctx, feat: torch.Tensor, hu: int, wu: int, sin_mode: int, *params: torch.Tensor) -> torch.Tensor:
        feat_c = T.checked_features(feat, params, INITQ_PARAM_NAMES, INITQ_PARAM_SHAPES, hu, wu, PAD_ROWS, " for decoder mode 3 with init_q")
        out, acts, packed, image, split, initq_split = train_forward_initq_split(feat_c, params, hu, wu, sin_mode)
        ctx.save_for_backward(feat_c, acts, packed, image, split, initq_split)
        ctx.size = (hu, wu)
        return out

    @staticmethod
    def backward(ctx, gout: torch.Tensor):
        feat, acts, packed, image, split, initq_split = ctx.saved_tensors
        d_feat, d_params = IT.backward_fused_initq(gout.contiguous(), feat, acts, packed, image, ctx.size,
                                                   need_feat_grad=ctx.needs_input_grad[0], split=split, initq_split=initq_split)
        return T.function_grads(ctx, d_feat, d_params, 4)


def decode_with_grad(decoder, feat: torch.Tensor, size: Sequence[int]) -> torch.Tensor:
    """``ImplicitDecoder(mode=3, init_q=True, compute="bf16x3", hip_initq_split_bf16=True, hip_autograd_initq_split_bf16=True)
    .forward(x, size, None)`` under autograd."""
    hu, wu = size
    return DecodeInitqSplitFunction.apply(feat, int(hu), int(wu), int(decoder.sin_mode), *T.named_params(decoder, INITQ_PARAM_NAMES))


# ---------------------------------------------------------------------------
# the emulation sheet (any device; the CPU tests and DESIGN.md 3.7g cite it)
# ---------------------------------------------------------------------------
def split_product(w: torch.Tensor, q: torch.Tensor, terms: Sequence[int] = (0, 1, 2)) -> torch.Tensor:
    """``sheets.split_matmul`` with its three terms selectable -- 0: w_lo . q_hi, 1: w_hi . q_lo, 2: w_hi . q_hi, added in that order.
    All three: ``split_matmul`` bit for bit.  Fewer: what a kernel that dropped a product would compute (the tests' negative control)."""
    if tuple(terms) == (0, 1, 2):
        return split_matmul(w.contiguous(), q)
    wh, wl = split_hi_lo(w.contiguous())
    qh, ql = split_hi_lo(q)
    parts = [(wl, qh), (wh, ql), (wh, qh)]
    out = None
    for t in terms:
        term = parts[t][0] @ parts[t][1]
        out = term if out is None else out + term
    return out


def split_forward_reference(sd: Dict[str, np.ndarray], feat: np.ndarray, size: Sequence[int]) -> Tuple[torch.Tensor, torch.Tensor]:
    """The split training forward in torch fp32, in RADIANS: (out [B,3,Hu,Wu], planes [4,2,256,N] = k_i, s_i).
    a by the kernels' fma sequence, E = sin a in fp32; ``s_0 = Q0 . E + bQ0``, ``PIX = Wx . x' + bK`` with the in-place
    ``x' = (E_hi + E_lo) * X`` and the two 256 x 256 products of layers 1..3 through ``split_matmul`` (torch matmuls, not the MFMA's
    summation order); the sines and the head in fp32."""
    f32 = torch.float32
    f = torch.from_numpy(np.asarray(feat, dtype=np.float32))
    get = S.tensor_getter(sd, "", f.device, f32)
    b, _, h, w = f.shape
    g = S.geometry(h, w, size, f.device)
    e = torch.sin(S.coordinate_fma(g, get("first_layer.0.weight", (UNFOLD, 3)), get("first_layer.0.bias", (UNFOLD, 1))))   # [576, n]
    eh, el = split_hi_lo(e)
    xp = (eh + el)[None] * S.gather_unfold(f, g)                                                    # [b, 576, n]
    wx, bk = S._stacked_k(get)
    pix = torch.stack([split_matmul(wx, xp[i]) for i in range(b)]) + bk                             # [b, 1024, n]
    s0 = split_matmul(get("Q.0.0.weight", (HIDDEN, UNFOLD)), e) + get("Q.0.0.bias", (HIDDEN, 1))    # [256, n]
    planes = [(torch.relu(pix[:, :HIDDEN]), s0[None].expand(b, HIDDEN, g.n))]
    q = planes[0][0] * torch.sin(s0)[None]
    for i in (1, 2, 3):
        wq = get(f"K.{i}.0.weight", (HIDDEN, HIDDEN + UNFOLD))[:, :HIDDEN].contiguous()
        qw = get(f"Q.{i}.0.weight", (HIDDEN, HIDDEN))
        k = torch.relu(torch.stack([split_matmul(wq, q[j]) for j in range(b)]) + pix[:, HIDDEN * i:HIDDEN * (i + 1)])
        s = torch.stack([split_matmul(qw, q[j]) for j in range(b)]) + get(f"Q.{i}.0.bias", (HIDDEN, 1))
        planes.append((k, s))
        q = k * torch.sin(s)
    out = S.head1x1(get, q, g)
    acts = torch.stack([torch.stack([k.permute(1, 0, 2).reshape(HIDDEN, -1), s.permute(1, 0, 2).reshape(HIDDEN, -1)]) for k, s in planes])
    return out, acts


def split_backward_reference(gout: torch.Tensor, feat: torch.Tensor, acts: torch.Tensor, params: Sequence[torch.Tensor],
                             size: Sequence[int], need_feat_grad: bool = True, terms: Sequence[int] = (0, 1, 2)
                             ) -> Tuple[Optional[torch.Tensor], List[torch.Tensor]]:
    """``initq_training.backward_from_saved_initq`` on GIVEN planes with the four transposed per-pixel products -- the chain's, dx' and
    t -- formed through ``split_product`` as bwd_layer_x3_kernel and initq_bwd_x3_kernel form them.  Everything else is that
    function's (fp32 ``acts``)."""
    return IT.backward_from_saved_initq(gout, feat, acts, params, size, need_feat_grad=need_feat_grad,
                                        product=lambda w_t, g_: split_product(w_t, g_, terms))
