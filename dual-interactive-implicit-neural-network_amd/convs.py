"""The 64-output convolutions of the encoder's kernel families as the Python layer drives them, stated once: the weight images
(``pack_conv_*``), which family runs a 3x3 layer on a B x H x W map (``conv_form``: the rule ``diinn_rdn_forward_ex`` owns), the
launch of one 3x3 layer in a given form (``launch_conv3x3``) and the F(4x4) kernel's split area (``w4_area``).  Their users are
the inference trunk (modules.RDN), the dense blocks under autograd (encoder_training) and the hoisted conv's input gradient
(training._conv_grads_native).  A leaf module: torch and the C ABI binding only.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _native


# ---------------------------------------------------------------------------
# weight images
# ---------------------------------------------------------------------------
def pack_conv_ksplit(weight: torch.Tensor) -> torch.Tensor:
    """Conv weight [64, Cin, kh, kw] (Cin % 64 == 0; 3x3 or 1x1) -> the layout ``diinn_conv_ksplit`` reads
    (include/diinn_hip.h): [half 2][wave 8][tap][group][lane 64][4] with cout = 32 half + (lane & 31) and
    input channel = wave*Cin/8 + 8 group + 2 e + (lane >> 5)."""
    co, cin, kh, kw = weight.shape
    if co != 64 or cin % 64 or (kh, kw) not in ((3, 3), (1, 1)):
        raise ValueError(f"unsupported convolution shape {tuple(weight.shape)}")
    taps, groups = kh * kw, cin // 64
    w = weight.detach().to(torch.float32).reshape(2, 32, 8, groups, 4, 2, taps)     # [half, i, wave, g, e, h, tap]
    return w.permute(0, 2, 6, 3, 5, 1, 4).reshape(-1)                               # [half, wave, tap, g, h, i, e]


def _winograd_weight(weight: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
    """U = G W G^T per (output, input) pair, [O, C, 3, 3] -> [O, C, R, R], in ``g``'s dtype as plain broadcast products and sums
    (left to right, (G W) first: the host packer's order for the decoder's hoisted conv) -- not an einsum, which would run a
    library GEMM per call (the training step re-packs the input gradient's weight whenever a parameter changed)."""
    w = weight.detach().to(g.dtype)
    r = g.shape[0]
    gi = [g[:, a].view(1, 1, r, 1) for a in range(3)]
    t = gi[0] * w[:, :, 0:1, :] + gi[1] * w[:, :, 1:2, :] + gi[2] * w[:, :, 2:3, :]          # [O, C, R, 3]
    gj = [g[:, b].view(1, 1, 1, r) for b in range(3)]
    return t[..., 0:1] * gj[0] + t[..., 1:2] * gj[1] + t[..., 2:3] * gj[2]                   # [O, C, R, R]


# G of F(2x2, 3x3): ``pack_conv_wino`` and the decoder's training image (training._fill_wpu_weight) transform with it
_WINO2_G = ((1.0, 0.0, 0.0), (0.5, 0.5, 0.5), (0.5, -0.5, 0.5), (0.0, 0.0, 1.0))


def pack_conv_wino(weight: torch.Tensor, dtype: torch.dtype = torch.float64) -> torch.Tensor:
    """3x3 conv weight [64, Cin, 3, 3] (Cin % 8 == 0) -> the Winograd F(2x2, 3x3) image ``diinn_conv_wino`` reads
    (include/diinn_hip.h): U = G W G^T per (output, input) pair, computed in float64 and rounded once, laid out
    [row i 4][chunk Cin/8][col j 4][half 2][lane 64][4] with cout = 32 half + (lane & 31) and input channel =
    8 chunk + 2 e + (lane >> 5); column j = 2 is stored negated."""
    co, cin, kh, kw = weight.shape
    if co != 64 or cin % 8 or (kh, kw) != (3, 3):
        raise ValueError(f"unsupported convolution shape {tuple(weight.shape)}")
    g = torch.tensor(_WINO2_G, dtype=dtype, device=weight.device)   # on the weight's device: 1.4 s for the trunk on the CPU, ms on the GPU
    u = _winograd_weight(weight, g).to(torch.float32)
    u[..., 2] = -u[..., 2]                                      # the kernel's input transform produces column 2 negated
    u = u.reshape(2, 32, cin // 8, 4, 2, 4, 4)                  # [half, m, chunk, e, h, i, j]
    return u.permute(5, 2, 6, 0, 4, 1, 3).reshape(-1)           # [i, chunk, j, half, h, m, e]


_WINO4_G = ((1 / 4, 0, 0), (-1 / 6, -1 / 6, -1 / 6), (-1 / 6, 1 / 6, -1 / 6), (1 / 24, 1 / 12, 1 / 6), (1 / 24, -1 / 12, 1 / 6), (0, 0, 1))


def pack_conv_wino4(weight: torch.Tensor, dtype: torch.dtype = torch.float64) -> torch.Tensor:
    """3x3 conv weight [64, Cin, 3, 3] (Cin % 8 == 0) -> the Winograd F(4x4, 3x3) image ``diinn_conv_wino4`` reads
    (include/diinn_hip.h): U = G W G^T (6x6 per (output, input) pair), computed in float64 and rounded once, laid out
    [wave 12][half 2][chunk Cin/8][q 3][lane 64][4] with position 6 i + j = 3 wave + q, cout = 32 half + (lane & 31)
    and input channel = 8 chunk + 2 e + (lane >> 5)."""
    co, cin, kh, kw = weight.shape
    if co != 64 or cin % 8 or (kh, kw) != (3, 3):
        raise ValueError(f"unsupported convolution shape {tuple(weight.shape)}")
    g = torch.tensor(_WINO4_G, dtype=dtype, device=weight.device)
    u = _winograd_weight(weight, g).to(torch.float32)
    u = u.reshape(2, 32, cin // 8, 4, 2, 12, 3)                 # [half, m, chunk, e, h, wave, q]
    return u.permute(5, 0, 2, 6, 4, 1, 3).reshape(-1)           # [wave, half, chunk, q, h, m, e]


def pack_conv_x3(weight: torch.Tensor) -> torch.Tensor:
    """Conv weight [64, Cin, k, k] (k = 3 or 1, Cin % 16 == 0) -> the split-bf16 image ``diinn_conv3x3_x3`` and the trunk's
    split-bf16 fusion layer read (include/diinn_hip.h): every weight as hi = bf16(w), lo = bf16(w - hi), laid out
    [group Cin/16][tap k*k][M-tile 2][hi, lo][lane 64][8 bf16] with cout = 32 mt + (lane & 31) and input channel =
    16 group + 8 (lane >> 5) + j; returned as float32 words (two bf16 each), k*k * 64 * Cin of them."""
    co, cin, kh, kw = weight.shape
    if co != 64 or cin % 16 or (kh, kw) not in ((3, 3), (1, 1)):
        raise ValueError(f"unsupported convolution shape {tuple(weight.shape)}")
    taps = kh * kw
    w = weight.detach().to(torch.float32)
    hi = w.to(torch.bfloat16)
    lo = (w - hi.to(torch.float32)).to(torch.bfloat16)
    parts = torch.stack([hi, lo], 0).reshape(2, 2, 32, cin // 16, 2, 8, taps)       # [part, mt, m, g, h, j, tap]
    img = parts.permute(3, 6, 1, 0, 4, 2, 5).contiguous()                           # [g, tap, mt, part, h, m, j]
    return img.view(torch.int16).reshape(-1, 2).view(torch.int32).reshape(-1).view(torch.float32)


# ---------------------------------------------------------------------------
# the split-bf16 trunk's emulation sheets (test infrastructure: plain torch on CPU tensors, no kernel is touched)
# ---------------------------------------------------------------------------
# The faults a sheet can carry (``fault=``): what a wrong split-format kernel would do, applied to the emulation so that a test
# can show that it would notice (tests/test_encoder_trunk_x3.py).  Never set outside tests.
X3_FAULTS = ("lo_vector",       # the lo half of ONE 8-channel vector (group 3, the middle pixel) of the last dense layer's output zeroed
             "lo_last_pixel",   # the lo halves of the map's last pixel zeroed in every dense layer's output
             "wlo_tail",        # w_lo . x_hi dropped for the last 16 input channels of the Cin = 512 layer
             "lo_layer",        # every lo half of the last dense layer's output zeroed
             "trunc")           # lo formed by truncation instead of round-to-nearest-even


def _bf16_rne(v: torch.Tensor) -> torch.Tensor:
    return v.to(torch.bfloat16).to(torch.float32)


def split_pair(v: torch.Tensor, fault: Optional[str] = None):
    """fp32 -> the split pair the kernels store: hi = bf16_rne(v), lo = bf16_rne(v - hi), both as float32."""
    hi = _bf16_rne(v)
    r = v - hi
    lo = (r.contiguous().view(torch.int32) & -65536).view(torch.float32) if fault == "trunc" else _bf16_rne(r)
    return hi, lo


def unpack_conv_x3(image: torch.Tensor, cin: int, k: int):
    """The inverse of ``pack_conv_x3``: its image of a [64, cin, k, k] weight -> (hi, lo) as float32 [64, cin, k, k]."""
    parts = image.contiguous().view(torch.int16).reshape(cin // 16, k * k, 2, 2, 2, 32, 8)    # [g, tap, mt, part, h, m, j]
    parts = parts.permute(3, 2, 5, 0, 4, 6, 1).contiguous().view(torch.bfloat16)              # [part, mt, m, g, h, j, tap]
    hi, lo = parts.reshape(2, 64, cin, k, k).to(torch.float32)
    return hi, lo


def split_planes_decode(xs: torch.Tensor):
    """The trunk's split activation buffer viewed as int16 [B, 72, 2, H*W, 8] ([b][group of 8 channels][hi, lo][pixel][j],
    channel = 8 group + j: csrc/diinn_conv_x3.hip) -> (hi, lo) as float32 [B, 576, H*W]."""
    b, groups, _, hw, _ = xs.shape
    v = xs.contiguous().view(torch.bfloat16).permute(2, 0, 1, 4, 3).reshape(2, b, 8 * groups, hw).to(torch.float32)
    return v[0], v[1]


def conv_x3_reference(x_hi, x_lo, weight, bias, padding, relu=True, residual=None, fault: Optional[str] = None):
    """The emulation sheet of one split-bf16 layer: the operands as bf16-exact float32 hi / lo parts, the three products
    w_lo.x_hi + w_hi.x_lo + w_hi.x_hi as float32 convolutions added in that order, then bias, ReLU and the residual in fp32
    (``conv3x3_x3_kernel`` / ``conv1x1_x3_kernel``; what it does not model is the order of the fp32 sums inside a product).
    Returns (v, hi, lo): the output as fp32 and as the split pair the kernel stores.  ``fault``: one of X3_FAULTS, tests only."""
    import torch.nn.functional as F
    w = weight.detach().to(torch.float32)
    w_hi, w_lo = split_pair(w)
    if fault == "wlo_tail" and w.shape[1] == 512:
        w_lo = w_lo.clone()
        w_lo[:, -16:] = 0
    v = F.conv2d(x_hi, w_lo, None, padding=padding) + F.conv2d(x_lo, w_hi, None, padding=padding)
    v = v + F.conv2d(x_hi, w_hi, None, padding=padding)
    v = v + bias.detach().to(torch.float32).view(1, -1, 1, 1)
    if relu:
        v = v.relu()
    if residual is not None:
        v = v + residual
    hi, lo = split_pair(v, fault)
    return v, hi, lo


def rdb_x3_reference(block, x, fault: Optional[str] = None):
    """The sheet of one residual dense block (modules.RDB) inside the split-bf16 trunk, from its fp32 input ``x`` [B,64,H,W]: the
    input split, eight dense layers that read and write split pairs only, the 1x1 fusion layer over all 576 channels plus ``x``.
    Returns (out, out_hi, out_lo, dense_hi, dense_lo): the block's fp32 output, its split pair, and the split pairs of the eight
    dense outputs as [B,512,H,W] -- what the trunk leaves in its fusion input, in groups 0..7 and in groups 8..71 of its split
    buffer.  ``fault``: one of X3_FAULTS, tests only."""
    hi, lo = split_pair(x, fault if fault == "trunc" else None)
    last = len(block.convs) - 1
    for c, layer in enumerate(block.convs):
        conv = layer.conv[0]
        _, h, l = conv_x3_reference(hi, lo, conv.weight, conv.bias, 1, fault=fault if fault in ("wlo_tail", "trunc") else None)
        if fault == "lo_last_pixel":
            l[:, :, -1, -1] = 0
        if c == last and fault == "lo_layer":
            l.zero_()
        if c == last and fault == "lo_vector":
            l[0, 24:32, l.shape[2] // 2, l.shape[3] // 2] = 0
        hi, lo = torch.cat([hi, h], 1), torch.cat([lo, l], 1)
    out, out_hi, out_lo = conv_x3_reference(hi, lo, block.LFF.weight, block.LFF.bias, 0, relu=False, residual=x,
                                            fault="trunc" if fault == "trunc" else None)
    return out, out_hi, out_lo, hi[:, 64:], lo[:, 64:]


# ---------------------------------------------------------------------------
# which kernel family runs a 3x3 layer, its image, its launch
# ---------------------------------------------------------------------------
def conv_form(b: int, h: int, w: int) -> str:
    """The trunk's rule (owner: diinn_rdn_forward_ex) for a 64-output 3x3 layer on a B x H x W map: "wino4" (F(4x4)) where
    diinn_rdn_wino4_applies, else "wino" (F(2x2)) from DIINN_ENC_WINO_MIN pixels, else "ksplit" (the split-K kernel)."""
    if _native.load().diinn_rdn_wino4_applies(b, h, w):
        return "wino4"
    return "wino" if b * h * w >= _native.debug_get("DIINN_ENC_WINO_MIN") else "ksplit"


def pack_conv3x3(weight: torch.Tensor, form: str) -> torch.Tensor:
    """The image of a 3x3 weight [64, Cin, 3, 3] that ``form``'s kernel reads."""
    return pack_conv_wino4(weight) if form == "wino4" else pack_conv_wino(weight) if form == "wino" else pack_conv_ksplit(weight)


def _ptr(t: Optional[torch.Tensor], offset: int = 0):
    return None if t is None else C.c_void_p(t.data_ptr() + 4 * offset)


WINO4_COUNTER_WORDS = 512   # DIINN_WINO4_COUNTER_BYTES / 4 (include/diinn_hip.h): the split area's arrival counters


def launch_conv3x3(form: str, stream, ws, b, h, w, inp, in_off, in_bs, cin, pk, bias, res, res_off, res_bs, out, out_off, out_bs, relu):
    """One 3x3 layer in ``form`` on ``stream`` through the trunk's single-layer entry point: ``pk`` is ``pack_conv3x3(weight, form)``,
    offsets and batch strides are in floats, ``ws`` is the split area of this (device, stream) (``w4_area``; "wino4" only)."""
    lib = _native.load()
    if form == "wino4":
        ws[:WINO4_COUNTER_WORDS].zero_()                         # the arrival counters, as the trunk does (never the sticky status word)
        _native.check(lib.diinn_conv_wino4_ws(stream, _ptr(inp, in_off), in_bs, cin, _ptr(pk), _ptr(bias), _ptr(res, res_off),
                                              res_bs, _ptr(out, out_off), out_bs, relu, b, h, w, _ptr(ws), ws.numel()),
                      "diinn_conv_wino4_ws")
    elif form == "wino":
        _native.check(lib.diinn_conv_wino(stream, _ptr(inp, in_off), in_bs, cin, _ptr(pk), _ptr(bias), _ptr(res, res_off),
                                          res_bs, _ptr(out, out_off), out_bs, relu, b, h, w), "diinn_conv_wino")
    else:
        _native.check(lib.diinn_conv_ksplit(stream, _ptr(inp, in_off), in_bs, cin, 9, _ptr(pk), _ptr(bias), _ptr(res, res_off),
                                            res_bs, _ptr(out, out_off), out_bs, None, 0, relu, b, h, w), "diinn_conv_ksplit")


# ---------------------------------------------------------------------------
# the F(4x4) kernel's split area
# ---------------------------------------------------------------------------
# 34.6 MB: control words + partial-output slabs, ONE per (device, stream), kept across forwards: its sticky status word then
# remembers a hand-off that ever gave up (handoff_status()); two streams never share slabs or tickets.  Process-wide: every
# user on that (device, stream) shares it (launches on one stream are ordered).
_w4_areas: dict = {}
_W4_AREAS_MAX = 16


def w4_area(device) -> torch.Tensor:
    floats = _native.load().diinn_conv_wino4_workspace_floats()
    if torch.cuda.is_current_stream_capturing():
        # inside a hipGraph capture the area comes from the graph's private pool and lives with the graph (its control
        # words are zeroed by a captured memset: a replay starts clean; a give-up is still NaN in that replay's output)
        ws = torch.empty(floats, dtype=torch.float32, device=device)
        ws[:1024].zero_()
        return ws
    key = (str(device), torch.cuda.current_stream(device).cuda_stream)
    ws = _w4_areas.get(key)
    if ws is None:
        while len(_w4_areas) >= _W4_AREAS_MAX:                   # streams come and go: the oldest area goes with them
            _w4_areas.pop(next(iter(_w4_areas)))
        ws = torch.empty(floats, dtype=torch.float32, device=device)
        ws[:1024].zero_()                                 # the control words, once (a forward re-zeroes only the counters)
        _w4_areas[key] = ws
    return ws


def handoff_status(clear: bool = True) -> int:
    """1 if the F(4x4) kernel's cross-workgroup hand-off has ever given up on one of this process' split areas (the
    features computed then, and since, are NaN: the failure is loud on the device already); synchronises the streams
    concerned.  ``clear`` re-arms the areas."""
    lib = _native.load()
    worst = 0
    for (dev, stream), ws in list(_w4_areas.items()):
        st = C.c_int(0)
        with torch.cuda.device(ws.device):
            _native.check(lib.diinn_conv_wino4_ws_status(C.c_void_p(stream), C.c_void_p(ws.data_ptr()), int(clear), C.byref(st)),
                          "diinn_conv_wino4_ws_status")
        worst = max(worst, st.value)
    return worst
