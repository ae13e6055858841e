"""Training path of the encoder's residual dense blocks (opt-in: ``RDN.hip_autograd``): autograd through the HIP kernels.

The reference trains the encoder by running ``RDB.forward`` (rdn.py:34-35: ``LFF(convs(x)) + x`` with ``RDB_Conv.forward``,
rdn.py:15-17: ``torch.cat((x, relu(conv(x))), 1)``) under autograd: per block 8 library convolutions and their data and weight
gradients, 8 ``torch.cat`` copies of the growing stack, everything saved.  Here one ``RDBFunction`` per block:

  forward   one dense buffer buf [B,576,H,W]; layer c is ONE launch of the trunk's single-layer entry point (diinn_conv_ksplit /
            diinn_conv_wino / diinn_conv_wino4_ws by the trunk's rule) reading buf[:, :64(c+1)] and writing group c+1 with
            ReLU; LFF is diinn_conv_ksplit with taps = 1 and res = x.  Saved: buf (the post-ReLU outputs are their own
            masks) and the parameters.
  backward  d_buf = W_LFF^T g_out (nine 1x1 launches, Cin = 64); then for j = 8..1 the full gradient of group j,
                D_j = d_buf[group j] + conv3x3(G[:, 64j:512]; Wt_j),   Wt_j[o, (c,co), ky, kx] = W_c[co, 64j+o, 2-ky, 2-kx], c = j..7
            -- ONE 64-output convolution with Cin = 64(8-j), a forward layer's shape on the forward's kernels -- gated into
            G[:, 64(j-1):64j] = D_j * [buf[group j] > 0] (diinn_relu_gate); d_x = g_out + d_buf[group 0] + conv3x3(G; Wt_0).
            Weight and bias gradients: diinn_conv_wgrad (fp32 MFMA GEMM over the pixel axis, the unfold gathered on the fly,
            split over pixel slices) + diinn_sum_parts.  No framework convolution, no atomics.

``rdb_backward_reference`` states the same gradients in device-agnostic tensor algebra (the convolutions from torch.nn.grad):
the CPU-tested formula sheet and the on-GPU cross-check, as ``training.backward_from_saved`` is for the decoder.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import _native, convs
from .convs import _ptr

G0 = 64                     # channels of a block's input and output
GROWTH = 64                 # channels every dense layer appends
LAYERS = 8                  # dense layers per block (config 'B')
DENSE = G0 + LAYERS * GROWTH   # 576: channels of the dense buffer
FORMS = ("auto", "ksplit", "wino", "wino4")
WGRAD_WORKGROUPS = 256      # workgroups a weight-gradient launch aims at (Cin / 64 channel blocks x pixel slices): one per CU


def block_params(rdb) -> List[torch.Tensor]:
    """(W_0, b_0, ..., W_7, b_7, W_LFF, b_LFF) of a modules.RDB, the argument order of RDBFunction after x."""
    out: List[torch.Tensor] = []
    for layer in rdb.convs:
        out += [layer.conv[0].weight, layer.conv[0].bias]
    return out + [rdb.LFF.weight, rdb.LFF.bias]


def block_applies(rdb) -> bool:
    """True for the config-'B' block shape RDBFunction covers: 8 dense 3x3 layers, G0 = G = 64, 1x1 fusion of 576 planes."""
    convs = [layer.conv[0] for layer in rdb.convs]
    return (len(convs) == LAYERS and tuple(rdb.LFF.weight.shape) == (G0, DENSE, 1, 1)
            and all(tuple(cv.weight.shape) == (GROWTH, G0 + c * GROWTH, 3, 3) and cv.padding == (1, 1) for c, cv in enumerate(convs)))


def transposed_weight(weights: Sequence[torch.Tensor], j: int) -> torch.Tensor:
    """Wt_j [64, 64(8-j), 3, 3] of D_j's convolution: Wt_j[o, 64(c-j)+co, ky, kx] = W_c[co, 64j+o, 2-ky, 2-kx] for c = j..7 --
    the slices of the 3x3 weights W_0..W_7 that read group j, flipped and transposed, stacked over the reading layers."""
    if not 0 <= j < LAYERS:
        raise ValueError(f"group {j} is read by no dense layer")
    lo = GROWTH * j
    return torch.cat([weights[c][:, lo:lo + GROWTH].flip(2, 3).permute(1, 0, 2, 3) for c in range(j, LAYERS)], 1).contiguous()


def rdb_backward_reference(g_out: torch.Tensor, buf: torch.Tensor, params: Sequence[torch.Tensor]
                           ) -> Tuple[torch.Tensor, List[torch.Tensor]]:
    """Gradients of one residual dense block given d(loss)/d(out): (d_x, [d W_0, d b_0, ..., d W_LFF, d b_LFF]).

    g_out [B,64,H,W]; buf [B,576,H,W] = (x, relu(conv_0), ..., relu(conv_7)), the block's dense buffer; params as block_params.
    With y_c = buf[group c+1] = relu(conv3x3(buf[:, :64(c+1)]; W_c) + b_c) and out = W_LFF buf + b_LFF + x:
        d_buf = W_LFF^T g_out;   for c = 7..0:  g_c = d_buf[group c+1] * [y_c > 0],  dW_c = g_c (*) buf[:, :64(c+1)],
        db_c = sum of g_c,  d_buf[:, :64(c+1)] += conv3x3^T(g_c; W_c);   d_x = g_out + d_buf[group 0]."""
    from torch.nn.grad import conv2d_input, conv2d_weight
    ws = list(params[0:2 * LAYERS:2])
    w_lff = params[2 * LAYERS]
    b = buf.shape[0]
    h, w = buf.shape[-2:]
    grads: List[Optional[torch.Tensor]] = [None] * (2 * LAYERS + 2)
    grads[2 * LAYERS] = conv2d_weight(buf, w_lff.shape, g_out)
    grads[2 * LAYERS + 1] = g_out.sum((0, 2, 3))
    d_buf = conv2d_input(buf.shape, w_lff, g_out).clone()
    for c in range(LAYERS - 1, -1, -1):
        cin = G0 + GROWTH * c
        g_c = d_buf[:, cin:cin + GROWTH] * (buf[:, cin:cin + GROWTH] > 0)
        grads[2 * c] = conv2d_weight(buf[:, :cin], ws[c].shape, g_c, padding=1)
        grads[2 * c + 1] = g_c.sum((0, 2, 3))
        d_buf[:, :cin] += conv2d_input((b, cin, h, w), ws[c], g_c, padding=1)
    return g_out + d_buf[:, :G0], grads


# ---------------------------------------------------------------------------
# packed weight images of a block, per kernel form
# ---------------------------------------------------------------------------
# (form, device, addresses of the block's 9 weights) -> (their versions, forward images [8] + LFF, transposed images [8] + the nine
# 1x1 images of W_LFF^T, the pinned weights).  Rebuilt when a version moves (an optimiser step, a load_state_dict); an entry PINS the
# weight tensors its key describes (as training._dgrad_pack does), so their addresses cannot be handed to other weights meanwhile.
_block_packs: Dict[tuple, tuple] = {}
BLOCK_PACKS_MAX = 128       # 16 blocks x the forms a multi-scale run alternates between, for a few models


def _packs(params: Sequence[torch.Tensor], form: str, dev, backward: bool):
    ws = [p.detach() for p in params[0:2 * LAYERS + 1:2]]        # W_0..W_7, W_LFF
    key = (form, str(dev)) + tuple(t.data_ptr() for t in ws)
    versions = tuple(t._version for t in ws)
    ent = _block_packs.pop(key, None)
    if ent is None or ent[0] != versions:
        ent = (versions, None, None, tuple(ws))
    if ent[1] is None:
        fwd = [convs.pack_conv3x3(ws[c], form) for c in range(LAYERS)] + [convs.pack_conv_ksplit(ws[LAYERS])]
        ent = (versions, fwd, ent[2], ent[3])
    if backward and ent[2] is None:
        bwd = [convs.pack_conv3x3(transposed_weight(ws, j), form) for j in range(LAYERS)]
        lff_t = ws[LAYERS].reshape(G0, LAYERS + 1, GROWTH).permute(1, 2, 0)          # [group, o, co] = W_LFF[co, 64 group + o]
        bwd += [convs.pack_conv_ksplit(lff_t[k].reshape(GROWTH, G0, 1, 1)) for k in range(LAYERS + 1)]
        ent = (versions, ent[1], bwd, ent[3])
    while len(_block_packs) >= BLOCK_PACKS_MAX:
        _block_packs.pop(next(iter(_block_packs)))
    _block_packs[key] = ent
    return ent[1], ent[2]


choose_form = convs.conv_form    # the trunk's rule, which training._conv_grads_native follows as well


class _Launcher:
    """One block's launches on the current stream of ``dev``: conv (3x3 in the block's form, or 1x1), gate, weight gradient."""

    def __init__(self, form: str, dev, b: int, h: int, w: int):
        self.lib = _native.load()
        self.form, self.dev, self.b, self.h, self.w = form, dev, b, h, w
        self.hw = h * w
        self.stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        self.ws = convs.w4_area(dev) if form == "wino4" else None    # the split area of this (device, stream)

    def conv3x3(self, inp, in_off, in_bs, cin, pk, bias, res, res_off, res_bs, out, out_off, out_bs, relu):
        convs.launch_conv3x3(self.form, self.stream, self.ws, self.b, self.h, self.w, inp, in_off, in_bs, cin, pk, bias,
                             res, res_off, res_bs, out, out_off, out_bs, relu)

    def conv1x1(self, inp, in_off, in_bs, cin, pk, bias, res, res_bs, out, out_off, out_bs):
        _native.check(self.lib.diinn_conv_ksplit(self.stream, _ptr(inp, in_off), in_bs, cin, 1, _ptr(pk), _ptr(bias), _ptr(res), res_bs,
                                                 _ptr(out, out_off), out_bs, None, 0, 0, self.b, self.h, self.w), "diinn_conv_ksplit")

    def gate(self, d, d_off, d_bs, y, y_off, y_bs, g, g_off, g_bs):
        _native.check(self.lib.diinn_relu_gate(self.stream, _ptr(d, d_off), d_bs, _ptr(y, y_off), y_bs, _ptr(g, g_off), g_bs,
                                               self.b, self.h, self.w), "diinn_relu_gate")

    def wgrad(self, g, g_off, g_bs, x, x_bs, cin, taps) -> torch.Tensor:
        """[64, cin * taps + 1]: the weight gradient in the weight's own order, and the bias gradient in the last column."""
        tiles = (self.b * self.hw + 31) // 32
        nsplit = max(1, min(tiles, -(-WGRAD_WORKGROUPS // (cin // 64))))
        n = 64 * (cin * taps + 1)
        part = torch.empty((nsplit, n), dtype=torch.float32, device=self.dev)
        _native.check(self.lib.diinn_conv_wgrad(self.stream, _ptr(g, g_off), g_bs, _ptr(x), x_bs, cin, taps, _ptr(part), nsplit,
                                                self.b, self.h, self.w), "diinn_conv_wgrad")
        out = torch.empty(n, dtype=torch.float32, device=self.dev)
        _native.check(self.lib.diinn_sum_parts(self.stream, _ptr(part), _ptr(out), 1, nsplit, n), "diinn_sum_parts")
        return out.view(64, cin * taps + 1)


def _check_input(x: torch.Tensor, params: Sequence[torch.Tensor], form: str) -> None:
    if form not in FORMS:
        raise ValueError(f"form must be one of {FORMS}, got {form!r}")
    if not x.is_cuda or x.dtype != torch.float32 or x.dim() != 4 or x.shape[1] != G0:
        raise NotImplementedError("RDBFunction covers CUDA float32 inputs [B,64,H,W]")
    if len(params) != 2 * LAYERS + 2:
        raise ValueError("RDBFunction takes (x, W_0, b_0, ..., W_7, b_7, W_LFF, b_LFF)")
    for c in range(LAYERS):
        if tuple(params[2 * c].shape) != (GROWTH, G0 + c * GROWTH, 3, 3) or tuple(params[2 * c + 1].shape) != (GROWTH,):
            raise NotImplementedError("RDBFunction covers the config-'B' block (G0 = G = 64, 8 dense 3x3 layers)")
    if tuple(params[2 * LAYERS].shape) != (G0, DENSE, 1, 1) or tuple(params[2 * LAYERS + 1].shape) != (G0,):
        raise NotImplementedError("RDBFunction covers the config-'B' block (1x1 fusion of 576 planes)")
    if any(p.device != x.device or p.dtype != torch.float32 for p in params):
        raise NotImplementedError("RDBFunction covers float32 parameters on the input's device")


def rdb_forward_buffer(x: torch.Tensor, params: Sequence[torch.Tensor], form: str = "auto") -> Tuple[torch.Tensor, torch.Tensor, str]:
    """The block's forward on the HIP kernels: (out [B,64,H,W], buf [B,576,H,W], the kernel form used)."""
    _check_input(x, params, form)
    x = x.detach().contiguous()
    b, _, h, w = x.shape
    dev = x.device
    hw = h * w
    if form == "auto":
        form = convs.conv_form(b, h, w)
    fwd, _ = _packs(params, form, dev, backward=False)
    buf = torch.empty((b, DENSE, h, w), dtype=torch.float32, device=dev)
    buf[:, :G0] = x
    out = torch.empty_like(x)
    with torch.cuda.device(dev):
        run = _Launcher(form, dev, b, h, w)
        for c in range(LAYERS):
            cin = G0 + GROWTH * c
            run.conv3x3(buf, 0, DENSE * hw, cin, fwd[c], params[2 * c + 1].detach().contiguous(), None, 0, 0,
                        buf, cin * hw, DENSE * hw, 1)
        run.conv1x1(buf, 0, DENSE * hw, DENSE, fwd[LAYERS], params[2 * LAYERS + 1].detach().contiguous(), x, G0 * hw,
                    out, 0, G0 * hw)
    return out, buf, form


def rdb_backward_fused(g_out: torch.Tensor, buf: torch.Tensor, params: Sequence[torch.Tensor], form: str,
                       need_x: bool = True, need_params: Optional[Sequence[bool]] = None
                       ) -> Tuple[Optional[torch.Tensor], List[Optional[torch.Tensor]]]:
    """``rdb_backward_reference``'s gradients on the HIP kernels (module docstring); ``need_params[i]`` False leaves grad i None,
    and with none needed no weight-gradient kernel is launched."""
    need_params = [True] * (2 * LAYERS + 2) if need_params is None else list(need_params)
    any_param = any(need_params)
    g_out = g_out.to(torch.float32).contiguous()
    b, _, h, w = buf.shape
    dev = buf.device
    hw = h * w
    _, bwd = _packs(params, form, dev, backward=True)
    zero = torch.zeros(64, dtype=torch.float32, device=dev)
    d_buf = torch.empty_like(buf)
    gates = torch.empty((b, LAYERS * GROWTH, h, w), dtype=torch.float32, device=dev)       # G: g_c at channel offset 64 c
    d_j = torch.empty((b, GROWTH, h, w), dtype=torch.float32, device=dev)
    grads: List[Optional[torch.Tensor]] = [None] * (2 * LAYERS + 2)
    d_x = None
    with torch.cuda.device(dev):
        run = _Launcher(form, dev, b, h, w)
        # d_buf = W_LFF^T g_out, group by group; group 0 takes the residual branch's g_out with it
        for k in range(LAYERS + 1):
            run.conv1x1(g_out, 0, G0 * hw, G0, bwd[LAYERS + k], zero, g_out if k == 0 else None, G0 * hw if k == 0 else 0,
                        d_buf, k * GROWTH * hw, DENSE * hw)
        run.gate(d_buf, LAYERS * GROWTH * hw, DENSE * hw, buf, LAYERS * GROWTH * hw, DENSE * hw,
                 gates, (LAYERS - 1) * GROWTH * hw, LAYERS * GROWTH * hw)
        for j in range(LAYERS - 1, 0, -1):
            run.conv3x3(gates, j * GROWTH * hw, LAYERS * GROWTH * hw, GROWTH * (LAYERS - j), bwd[j], zero,
                        d_buf, j * GROWTH * hw, DENSE * hw, d_j, 0, GROWTH * hw, 0)
            run.gate(d_j, 0, GROWTH * hw, buf, j * GROWTH * hw, DENSE * hw, gates, (j - 1) * GROWTH * hw, LAYERS * GROWTH * hw)
        if need_x:
            d_x = torch.empty((b, G0, h, w), dtype=torch.float32, device=dev)
            run.conv3x3(gates, 0, LAYERS * GROWTH * hw, LAYERS * GROWTH, bwd[0], zero, d_buf, 0, DENSE * hw, d_x, 0, G0 * hw, 0)
        if any_param:
            for c in range(LAYERS):
                if not (need_params[2 * c] or need_params[2 * c + 1]):
                    continue
                cin = G0 + GROWTH * c
                dw = run.wgrad(gates, c * GROWTH * hw, LAYERS * GROWTH * hw, buf, DENSE * hw, cin, 9)
                if need_params[2 * c]:
                    grads[2 * c] = dw[:, :cin * 9].reshape(GROWTH, cin, 3, 3)
                if need_params[2 * c + 1]:
                    grads[2 * c + 1] = dw[:, cin * 9]
            if need_params[2 * LAYERS] or need_params[2 * LAYERS + 1]:
                dw = run.wgrad(g_out, 0, G0 * hw, buf, DENSE * hw, DENSE, 1)
                if need_params[2 * LAYERS]:
                    grads[2 * LAYERS] = dw[:, :DENSE].reshape(G0, DENSE, 1, 1)
                if need_params[2 * LAYERS + 1]:
                    grads[2 * LAYERS + 1] = dw[:, DENSE]
    return d_x, grads


class RDBFunction(torch.autograd.Function):
    """``RDBFunction.apply(x, W_0, b_0, ..., W_7, b_7, W_LFF, b_LFF, form="auto")``: one residual dense block (config 'B', fp32,
    CUDA) under autograd on the HIP kernels.  ``form`` forces the kernel family of the 3x3 layers (tests; "auto": the trunk's rule)."""

    @staticmethod
    def forward(ctx, x, *args):
        form = "auto"
        if args and isinstance(args[-1], str):
            form, args = args[-1], args[:-1]
        params = args
        out, buf, form = rdb_forward_buffer(x, params, form)
        ctx.save_for_backward(buf, *params)
        ctx.form = form
        ctx.n_extra = 0 if len(args) == len(ctx.needs_input_grad) - 1 else 1
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_out):
        buf, *params = ctx.saved_tensors
        need = ctx.needs_input_grad
        d_x, grads = rdb_backward_fused(g_out, buf, params, ctx.form, need_x=need[0], need_params=need[1:1 + len(params)])
        return (d_x, *grads, *([None] * ctx.n_extra))
