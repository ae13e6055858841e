"""Mode 3 (``init_q=False``) under autograd with the per-pixel chain in split-bf16 arithmetic -- the opt-in
``ImplicitDecoder.hip_autograd_split_bf16`` together with ``compute="bf16x3"``.

The step of ``training.DecodeMode3Function`` with two kernels exchanged and one image added:

  image     the SPLIT TRAINING image (csrc/diinn_layout.h): the three per-pixel layers, and their transposes, as hi/lo bf16 pieces in
            section WLX's layout, filled on the device from the gathered training image (``diinn_pack_split_train``) once per weight
            version and cached beside ``training.pack_on_device``'s image under the same key rule (``pack_split_on_device``).
  forward   diinn_precompute_P_wpu as before, then decode_bf16x3_kernel<SIN | X3_SAVE> (``diinn_decode_train_fwd_x3``): every
            256 x 256 product is  W_lo.q_hi + W_hi.q_lo + W_hi.q_hi  on v_mfma_f32_32x32x16_bf16 with fp32 accumulation;
            hi = bf16(v), lo = bf16(v - hi).  It writes the same fp32 planes k_i, s_i (radians) as decode_kernel<SAVE>.
  backward  ``training.backward_fused(..., split=image)``: the chain g_q,i-1 = Wq_i^T g_a,i + Qw_i^T g_s,i on 3 x bwd_layer_x3_kernel
            (``diinn_backward_data_x3``) in the same arithmetic; the planes G_i, q_i it leaves are fp32 as before, and everything behind
            them -- the plane GEMMs, the rowdots, the cell sums, the conv gradients -- is unchanged.

Because the planes keep the fp32 contract the two forwards and the two backwards mix: ``train_forward_split`` + ``backward_fused``
without ``split`` is the split forward under the fp32 backward (the tests' bisecting tool).

The EMULATION SHEET (``split_forward_reference``, ``split_chain_backward_reference``) states the same arithmetic in torch fp32 on any
device, in the kernels' order of products (the two small ones first, the leading one last).  It is what the CPU tests hold against
the float64 oracle.  What an end-to-end gradient comparison cannot hold is the ReLU kink: a modulation pre-activation within the
split rounding of zero lands on the other side, and the gate is discontinuous there (DESIGN.md 3.7f has the measured case)."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _native
from . import training as T
from .sheets import split_hi_lo, split_matmul  # noqa: F401  (the sheet's two primitives; cited here by tests and DESIGN.md 3.7f)
from .training import HIDDEN, PARAM_NAMES, PARAM_SHAPES


# ---------------------------------------------------------------------------
# the split training image
# ---------------------------------------------------------------------------
def split_train_floats() -> int:
    return int(_native.load().diinn_split_train_floats())


def pack_split_host(image: np.ndarray) -> np.ndarray:
    """Host twin of the device packer: a host image holding sections WL and WLT (``decoder.pack_state_dict(sd).numpy()``) -> the
    split training image, float32 [2 * 393,216] whose bytes are the bf16 pieces."""
    image = np.ascontiguousarray(image, dtype=np.float32)
    out = np.empty(split_train_floats(), dtype=np.float32)
    _native.check(_native.load().diinn_pack_split_train_host(_native.fptr(image), _native.fptr(out)), "diinn_pack_split_train_host")
    return out


def pack_split_on_device(params: Sequence[torch.Tensor]) -> torch.Tensor:
    """Reference-ordered parameter tensors (PARAM_NAMES, mode 3's shapes) on a GPU -> the split training image on that GPU, from
    ``training.pack_on_device``'s gathered image.  Kept, like that image, while no parameter has been modified: the key is the
    parameters' (address, version) pairs, and the entry pins the tensors it describes."""
    def build():
        packed = T.pack_on_device(params)
        split = torch.empty(split_train_floats(), dtype=torch.float32, device=packed.device)
        with _native.launcher(packed.device) as run:
            run("diinn_pack_split_train", packed, split)
        return split
    return T.kept("split", T.weights_key(params), params, build)


# ---------------------------------------------------------------------------
# forward and the autograd function
# ---------------------------------------------------------------------------
def train_forward_split(feat_c: torch.Tensor, params: Sequence[torch.Tensor], hu: int, wu: int, sin_mode: int):
    """The split training forward on a contiguous fp32 CUDA ``feat_c``: ``training.train_forward_mode3`` with the split image, i.e.
    the hoisted conv (diinn_precompute_P_wpu), then decode_bf16x3_kernel<SIN | X3_SAVE> (diinn_decode_train_fwd_x3).
    Returns (out, acts [4,T,512,32], packed image, split image)."""
    packed = T.pack_on_device(params)
    split = pack_split_on_device(params)
    out, acts = T.train_forward_mode3(feat_c, packed, hu, wu, sin_mode, split=split)
    return out, acts, packed, split


class DecodeMode3SplitFunction(torch.autograd.Function):
    """out = decoder(feat) with the per-pixel chain in split-bf16 arithmetic both ways, differentiable in feat and the 18 parameter
    tensors: ``training.DecodeMode3Function`` on diinn_decode_train_fwd_x3 / diinn_backward_data_x3."""

    @staticmethod
    def forward(ctx, feat: torch.Tensor, hu: int, wu: int, sin_mode: int, *params: torch.Tensor) -> torch.Tensor:
        feat_c = T.checked_features(feat, params, PARAM_NAMES, PARAM_SHAPES, hu, wu, 2 * HIDDEN, " for decoder mode 3")
        out, acts, packed, split = train_forward_split(feat_c, params, hu, wu, sin_mode)
        ctx.save_for_backward(feat_c, acts, packed, split, *[p_.detach() for p_ in params])
        ctx.size = (hu, wu)
        return out

    @staticmethod
    def backward(ctx, gout: torch.Tensor):
        feat, acts, packed, split, *params = ctx.saved_tensors
        d_feat, d_params = T.backward_fused(gout.contiguous(), feat, acts, params, packed, ctx.size,
                                            need_feat_grad=ctx.needs_input_grad[0], split=split)
        return T.function_grads(ctx, d_feat, d_params, 4)


def decode_with_grad(decoder, feat: torch.Tensor, size: Sequence[int]) -> torch.Tensor:
    """``ImplicitDecoder.forward(x, size, None)`` under autograd for mode 3, ``init_q=False``, ``compute="bf16x3"`` with
    ``hip_autograd_split_bf16`` set."""
    hu, wu = size
    return DecodeMode3SplitFunction.apply(feat, int(hu), int(wu), int(decoder.sin_mode), *T.named_params(decoder, PARAM_NAMES))


# ---------------------------------------------------------------------------
# the emulation sheet (any device; the CPU tests and DESIGN.md 3.7f cite it)
# ---------------------------------------------------------------------------
def split_forward_reference(sd: Dict[str, np.ndarray], feat: np.ndarray, size: Sequence[int]) -> Tuple[torch.Tensor, torch.Tensor]:
    """The split training forward in torch fp32 on the CPU: (out [B,3,Hu,Wu], planes [4,2,256,N] = k_i, s_i in radians).
    P = conv3x3(feat; Wx) + bK per LR cell, replicated to the cell's pixels (the hoisted form the kernels run); layer 0, the seeds,
    the sines and the head in fp32; the two 256 x 256 products of layers 1..3 through ``split_matmul``."""
    p = {k: torch.from_numpy(np.asarray(v, dtype=np.float32)) for k, v in sd.items()}
    f = torch.from_numpy(np.asarray(feat, dtype=np.float32))
    b, _, h, w = f.shape
    hu, wu = int(size[0]), int(size[1])
    n = b * hu * wu
    idx_h, rel_h, idx_w, rel_w, ratio = T.coordinate_tensors(h, w, hu, wu, torch.device("cpu"))
    bk = torch.cat([p[f"K.{i}.0.bias"] for i in range(4)])
    pc = torch.nn.functional.conv2d(f, T._hoisted_conv_weight(p), bk, padding=1)              # [B,1024,H,W]
    pp = pc[:, :, idx_h][:, :, :, idx_w].permute(1, 0, 2, 3).reshape(4 * HIDDEN, n)            # per HR pixel
    syn = torch.empty((3, b, hu, wu), dtype=torch.float32)
    syn[0] = rel_h[None, :, None]
    syn[1] = rel_w[None, None, :]
    syn[2] = ratio
    acts = torch.empty((4, 2, HIDDEN, n), dtype=torch.float32)
    k = torch.relu(pp[:HIDDEN])
    s = p["Q.0.0.weight"].reshape(HIDDEN, 3) @ syn.reshape(3, n) + p["Q.0.0.bias"][:, None]
    acts[0, 0], acts[0, 1] = k, s
    q = k * torch.sin(s)
    for i in (1, 2, 3):
        wq = p[f"K.{i}.0.weight"].reshape(HIDDEN, -1)[:, :HIDDEN]
        k = torch.relu(split_matmul(wq, q) + pp[i * HIDDEN:(i + 1) * HIDDEN])
        s = split_matmul(p[f"Q.{i}.0.weight"].reshape(HIDDEN, HIDDEN), q) + p[f"Q.{i}.0.bias"][:, None]
        acts[i, 0], acts[i, 1] = k, s
        q = k * torch.sin(s)
    out = p["last_layer.weight"].reshape(3, HIDDEN) @ q + p["last_layer.bias"][:, None]
    return out.view(3, b, hu, wu).permute(1, 0, 2, 3).contiguous(), acts


def split_chain_backward_reference(gout: torch.Tensor, feat: torch.Tensor, acts: torch.Tensor, params: Sequence[torch.Tensor],
                                   size: Sequence[int], need_feat_grad: bool = True
                                   ) -> Tuple[Optional[torch.Tensor], List[torch.Tensor]]:
    """``training.backward_from_saved`` with the chain product g_q,i-1 = Wq_i^T g_a,i + Qw_i^T g_s,i formed as bwd_layer_x3_kernel
    forms it: each of the two products through ``split_matmul``, then their sum.  Everything else is that function's (fp32 ``acts``)."""
    def chain(wq_t, g_a, qw_t, g_s):
        return split_matmul(wq_t.contiguous(), g_a) + split_matmul(qw_t.contiguous(), g_s)
    return T.backward_from_saved(gout, feat, acts, params, size, need_feat_grad=need_feat_grad, chain=chain)
