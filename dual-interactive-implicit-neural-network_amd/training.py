"""Training path of the decoder, modes 1-3: autograd through the HIP kernels.

The reference trains by calling ``ImplicitDecoder.forward(x, size, bsize=None)`` with autograd on
(diinn.py:170-171 -> step(), :132-139; caller SRLitModule.training_step, sr_module.py:127-129), which
records ~30 ATen ops per call on the materialised [B,576,Hu,Wu] tensor.  Here:

  forward   precompute_P_kernel, then decode_kernel<SAVE> (C ABI ``diinn_decode_train_fwd``): the fused
            inference kernel that additionally writes every layer's rectified modulation k_i and sine
            argument s_i as [channel][pixel] planes -- all the backward pass needs.
  backward  ``backward_fused``: the per-pixel chain (gates and the transposed stacked GEMMs
            g_q[i-1] = Wq_i^T g_a + Qw_i^T g_s) runs on 3 x bwd_layer_kernel (C ABI
            ``diinn_backward_data``; the head's gates are computed inside layer 3's kernel), which leave
            the gate gradients G_i and the activations q_i as tiled planes; every parameter gradient is
            then one GEMM over the pixel axis per layer (plane_gemm_lds_kernel, split-K, no atomics),
            two skinny products (plane_rowdot_kernel), a per-cell segment sum (cell_sum_kernel) and the
            3x3 conv's gradients on the library's kernels as well (``_conv_grads_native``: unfold + the
            plane GEMM for the weight, the encoder's convolution kernels for the input).
            ``backward_from_saved`` states the same gradients in device-agnostic tensor algebra (the
            conv's from torch.nn.grad); it is the unit-tested formula sheet (CPU, against the
            reference's own .grad fixtures) and the on-GPU cross-check of the fused path.  The forward
            has no CPU form.

Modes 1 and 2 (diinn.py:116-131; the paper's ablations): the modulation chain k_i depends on the LR cell only, so the forward is
precompute_P, cell_chain_kernel, decode_kernel<KPART=false, SAVE> (``diinn_decode_train_fwd_qonly``) and the backward is the
per-pixel chain without its modulation half (``diinn_backward_data_qonly``), the cell sums, then cell_chain_kernel's scheme run
backwards (``diinn_cell_chain_bwd``): ``backward_fused_modes12``, with ``backward_from_saved_modes12`` as its formula sheet.

Weights change every optimiser step, so the packed image is rebuilt on the device each forward by one
gather through a permutation index derived once from the host packer (``pack_gather_index``).
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _native, convs

HIDDEN = 256
IN_CHANNELS = 64
UNFOLD = IN_CHANNELS * 9

# the reference's registration order (ImplicitDecoder.__init__, diinn.py:73-80,92)
PARAM_NAMES: List[str] = (
    [f"K.{i}.0.{t}" for i in range(4) for t in ("weight", "bias")]
    + [f"Q.{i}.0.{t}" for i in range(4) for t in ("weight", "bias")]
    + ["last_layer.weight", "last_layer.bias"]
)
PARAM_SHAPES: Dict[str, Tuple[int, ...]] = {
    "K.0.0.weight": (HIDDEN, UNFOLD, 1, 1), "K.0.0.bias": (HIDDEN,),
    **{f"K.{i}.0.weight": (HIDDEN, HIDDEN + UNFOLD, 1, 1) for i in (1, 2, 3)},
    **{f"K.{i}.0.bias": (HIDDEN,) for i in (1, 2, 3)},
    "Q.0.0.weight": (HIDDEN, 3, 1, 1), "Q.0.0.bias": (HIDDEN,),
    **{f"Q.{i}.0.weight": (HIDDEN, HIDDEN, 1, 1) for i in (1, 2, 3)},
    **{f"Q.{i}.0.bias": (HIDDEN,) for i in (1, 2, 3)},
    "last_layer.weight": (3, HIDDEN, 1, 1), "last_layer.bias": (3,),
}


def param_shapes(mode: int = 3) -> Dict[str, Tuple[int, ...]]:
    """PARAM_SHAPES for decoder ``mode``: modes 2 and 3 share them; mode 1's K.1..3 see k alone, [256,256,1,1] (diinn.py:53-60);
    mode 4 is mode 3 with the 3x3 head, ``last_layer.weight`` [3,256,3,3] (diinn.py:89-90)."""
    if mode == 4:
        return {**PARAM_SHAPES, "last_layer.weight": (3, HIDDEN, 3, 3)}
    if mode != 1:
        return PARAM_SHAPES
    return {**PARAM_SHAPES, **{f"K.{i}.0.weight": (HIDDEN, HIDDEN, 1, 1) for i in (1, 2, 3)}}


# backward_fused calls no framework convolution, GEMM or reduction of partials: the A/B runs that settled that are in DESIGN_HISTORY.md.
WGRAD_KSPLIT = 64          # pixel-axis splits of the weight-gradient GEMM: 4 output blocks x 64 = one workgroup per CU
ROWDOT_SPLITS = 1024       # workgroups of the skinny products (HBM-bound)

GEOMETRY_CACHE_ENTRIES = 8


# ---------------------------------------------------------------------------
# the caches of the training paths (this module's and those of the modules that build on it)
# ---------------------------------------------------------------------------
_kept: Dict[str, tuple] = {}                       # slot -> (key, value, the tensors the key describes)


def weights_key(tensors: Sequence[torch.Tensor]) -> tuple:
    """What identifies the values of ``tensors`` while they are alive: their (address, version) pairs."""
    return tuple((t.data_ptr(), t._version) for t in tensors)


def kept(slot: str, key, pins: Sequence[torch.Tensor], build):
    """The rule "keep the last image while no parameter has changed", stated once: the value ``build()`` returned for ``key`` the
    last time ``slot`` was asked, or a new one when the key differs.  The entry PINS ``pins``, the tensors the key describes: while
    it is cached their addresses cannot be handed to other weights with equal version counts.
    (What a key contains is its caller's: a write through ``.data`` bumps no ``_version`` and none of them sees it -- to change
    that, change the callers' keys through ``weights_key``.)"""
    ent = _kept.get(slot)
    if ent is None or ent[0] != key:
        ent = _kept[slot] = (key, build(), tuple(t.detach() for t in pins))
    return ent[1]


def lru(cache: dict, key, build):
    """``cache[key]``, built on a miss, in a small LRU (GEOMETRY_CACHE_ENTRIES; a hit becomes the newest entry): the per-shape
    constants of the backward passes -- training revisits a handful of shapes, one per scale."""
    value = cache.pop(key, None)
    if value is None:
        value = build()
        while len(cache) >= GEOMETRY_CACHE_ENTRIES:
            cache.pop(next(iter(cache)))
    cache[key] = value
    return value


_index_dev: Dict[tuple, torch.Tensor] = {}


def index_on(dev, name, index) -> torch.Tensor:
    """The gather index ``index()`` (a CPU tensor its maker keeps) on ``dev``: copied once per (name, device)."""
    key = (name, str(dev))
    if key not in _index_dev:
        _index_dev[key] = index().to(dev)
    return _index_dev[key]


def _layout(mode: int) -> int:
    """Weight layout of the packed body image: 1 (mode 1) or 3 (modes 2 and 3; mode 4, whose body image is mode 3's with a zero 1x1
    head -- its 3x3 head is an image of its own, mode4_training.py)."""
    if mode not in (1, 2, 3, 4):
        raise ValueError(f"the training path covers decoder modes 1-4, got {mode}")
    return 1 if mode == 1 else 3


def position_state_dict(names: Sequence[str], shapes: Dict[str, Tuple[int, ...]]) -> Tuple[Dict[str, np.ndarray], int]:
    """({name: fp32 array of ``shapes[name]`` whose elements are their own 1-based position in the tensors flattened in
    ``names`` order}, the element count): packing it and reading the positions back gives a packer's permutation (exact in fp32)."""
    sd, pos = {}, 1
    for name in names:
        n = int(np.prod(shapes[name]))
        sd[name] = np.arange(pos, pos + n, dtype=np.float32).reshape(shapes[name])
        pos += n
    assert pos - 1 < (1 << 24)
    return sd, pos - 1


def gather_index(packed: np.ndarray, total: int, blank: Sequence[Tuple[int, int]], what: str, of: str = "reference",
                 need: Optional[np.ndarray] = None) -> torch.Tensor:
    """int64 [image floats]: image[i] = flat[index[i]], from ``packed``, the image a host packer made of ``position_state_dict``'s
    ``total`` elements; ``flat`` is those tensors flattened in order followed by one 0.0.  The (offset, size) float ranges
    ``blank`` (derived values, a validity word) and the padding point at the appended zero.  Raises unless the rest is a
    permutation that references every element (``need``: a mask of the elements that must be; default all): ``what`` / ``of``
    name the image and its tensors in the two messages."""
    idx = np.rint(packed).astype(np.int64) - 1
    for off, size in blank:
        idx[off:off + size] = -1
    if idx.max() >= total or idx.min() < -1:
        raise RuntimeError(f"{what} is not a permutation of the {of} tensors")
    used = np.zeros(total, bool)
    used[idx[idx >= 0]] = True
    if not (used.all() if need is None else used[need].all()):
        raise RuntimeError(f"{what} does not reference every " + ("parameter element" if need is None else "element it is built from"))
    idx[idx < 0] = total                                # the appended zero
    return torch.from_numpy(idx)


DERIVED_SECTIONS = (7, 9, 10, 11, 12, 13, 14, 15, 16)           # inference-only sections of the DIINN image: derived values, no gather


def derived_ranges() -> List[Tuple[int, int]]:
    """The float ranges of a DIINN-layout image that a gather leaves empty: the derived sections and the validity word behind bL
    (DIINN_PACKED_MAGIC), which reads as zero in a gathered image: the inference entry points, which read the derived sections,
    then answer NaN instead of decoding with empty weights."""
    return [_section(i) for i in DERIVED_SECTIONS] + [(_section(6)[0] + 3, 1)]


_gather_index_cpu: Dict[int, torch.Tensor] = {}          # keyed by weight layout: 1 (mode 1) or 3 (modes 2 and 3)


def pack_gather_index(mode: int = 3) -> torch.Tensor:
    """int64 [packed floats]: packed[i] = flat[index[i]] where ``flat`` is the 18 reference tensors
    flattened in PARAM_NAMES order followed by one 0.0 (padding and the bf16 section point at it).
    Derived by packing a state dict whose values are their own flat position (exact in fp32).
    Mode 1 (K.1..3 are [256,256]): the feature columns the host packer widens them with are zeros, so
    those places -- layers 1..3 of the hoisted conv -- point at the appended zero as well."""
    layout = _layout(mode)
    if layout not in _gather_index_cpu:
        from .decoder import pack_state_dict
        sd, total = position_state_dict(PARAM_NAMES, param_shapes(layout))
        _gather_index_cpu[layout] = gather_index(pack_state_dict(sd, mode=layout).numpy(), total, derived_ranges(), "packed image")
    return _gather_index_cpu[layout]


def pack_on_device(params: Sequence[torch.Tensor], mode: int = 3) -> torch.Tensor:
    """Reference-ordered parameter tensors (PARAM_NAMES) on a GPU -> packed image on that GPU.
    The last image is kept while no parameter has been modified (a training step decodes once per
    scale with the same weights, sr_module.py:116-121).  ``mode`` 1: the tensors have mode 1's shapes."""
    return kept("packed", (_layout(mode), *weights_key(params)), params, lambda: _pack_on_device(params, mode))


_section_cache: Dict[int, Tuple[int, int]] = {}


def _section(i: int) -> Tuple[int, int]:
    if i not in _section_cache:
        off, size = C.c_size_t(), C.c_size_t()
        _native.check(_native.load().diinn_packed_section(i, C.byref(off), C.byref(size)), "diinn_packed_section")
        _section_cache[i] = (off.value, size.value)
    return _section_cache[i]


def _hoisted_conv_weight(p: Dict[str, torch.Tensor], mode: int = 3) -> torch.Tensor:
    """Wx [1024,64,3,3] of P = conv3x3(feat; Wx) + bK: the unfold columns of the four K weights, stacked over the layers.
    Mode 1: K.1..3 have no feature columns (P_i = bK_i there): Wx is K.0's [256,64,3,3] alone."""
    k0 = p["K.0.0.weight"].reshape(HIDDEN, UNFOLD)
    if mode == 1:
        return k0.reshape(HIDDEN, IN_CHANNELS, 3, 3).contiguous()
    wx = torch.cat([k0] + [p[f"K.{i}.0.weight"].reshape(HIDDEN, HIDDEN + UNFOLD)[:, HIDDEN:] for i in (1, 2, 3)], 0)
    return wx.reshape(4 * HIDDEN, IN_CHANNELS, 3, 3).contiguous()


def _fill_wpu(packed: torch.Tensor, params: Sequence[torch.Tensor], mode: int = 3) -> None:
    """Section 13 (WPU) of a gathered image, on the device (what diinn_precompute_P_wpu, the training forward's hoisted conv on the
    fp32 Winograd kernel, reads): U = G Wx G^T per (output, input) pair in float64 in the host
    packer's own operation order (csrc/diinn_host.cpp: (G g) first, then (.) G^T, sums left to right), rounded once, column 2
    negated, laid out [mt 32][row i 4][sg 8][col j 4][lane 64][e 4] -- bit-identical to diinn_pack_weights' section -- and
    the validity word DIINN_PACKED_MAGIC_WPU ("this training image holds WPU and nothing else derived")."""
    w = _hoisted_conv_weight({name: t.detach() for name, t in zip(PARAM_NAMES, params)}, mode).to(torch.float64)
    if mode == 1:                                                # layers 1..3 of the conv are zero (the host packer's widened K.i)
        w = torch.cat([w, w.new_zeros((3 * HIDDEN, IN_CHANNELS, 3, 3))], 0)
    _fill_wpu_weight(packed, w)


def _fill_wpu_weight(packed: torch.Tensor, w: torch.Tensor) -> None:
    """``_fill_wpu`` for any 1024-output 3x3 weight ``w`` [1024,64,3,3] (the MetaSR training image brings its own: metasr_training.py)."""
    u = convs._winograd_weight(w, torch.tensor(convs._WINO2_G, dtype=torch.float64, device=w.device))   # [O, C, i 4, j 4]
    u[..., 2] = -u[..., 2]
    u = u.to(torch.float32).reshape(32, 32, 8, 4, 2, 4, 4)                                   # [mt, m, sg, e, h, i, j]
    off, size = _section(13)
    packed[off:off + size] = u.permute(0, 5, 2, 6, 4, 1, 3).reshape(-1)                      # [mt, i, sg, j, h, m, e]
    word = _section(6)[0] + 3
    packed[word:word + 1].view(torch.int32).fill_(_native.PACKED_MAGIC_WPU)


def _pack_on_device(params: Sequence[torch.Tensor], mode: int = 3) -> torch.Tensor:
    dev = params[0].device
    flat = torch.cat([p.detach().reshape(-1).to(torch.float32) for p in params] + [torch.zeros(1, device=dev)])
    packed = flat.index_select(0, index_on(dev, _layout(mode), lambda: pack_gather_index(mode)))
    _fill_wpu(packed, params, mode)
    return packed


# ---------------------------------------------------------------------------
# coordinates as tensors (host tables from the C ABI, bit-exact with the kernels)
# ---------------------------------------------------------------------------
def coordinate_tensors(h: int, w: int, hu: int, wu: int, device) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, float]:
    from .decoder import axis_tables
    lib = _native.load()
    small = bool(lib.diinn_uses_small_output_kernel(hu, wu))
    idx_h, rel_h = axis_tables(h, hu, small)
    idx_w, rel_w = axis_tables(w, wu, small)
    ratio = float(np.float32((h * w) / (hu * wu)))
    return (torch.from_numpy(idx_h.astype(np.int64)).to(device), torch.from_numpy(rel_h).to(device),
            torch.from_numpy(idx_w.astype(np.int64)).to(device), torch.from_numpy(rel_w).to(device), ratio)


# ---------------------------------------------------------------------------
# backward from the saved planes (device-agnostic tensor algebra)
# ---------------------------------------------------------------------------
def _cell_sum(g: torch.Tensor, b: int, hu: int, wu: int, h: int, w: int,
              idx_h: torch.Tensor, idx_w: torch.Tensor) -> torch.Tensor:
    """g [C, B*Hu*Wu] -> [B, C, H, W]: sum over the HR pixels of every LR cell (adjoint of the nearest-exact
    replication, diinn.py:168), as two one-hot GEMMs so the summation order is fixed."""
    c = g.shape[0]
    mw = torch.zeros((wu, w), dtype=g.dtype, device=g.device)
    mw[torch.arange(wu, device=g.device), idx_w] = 1
    mh = torch.zeros((h, hu), dtype=g.dtype, device=g.device)
    mh[idx_h, torch.arange(hu, device=g.device)] = 1
    t = g.reshape(c * b * hu, wu) @ mw                       # [C*B*Hu, W]
    t = torch.matmul(mh, t.view(c * b, hu, w))               # [C*B, H, W]
    return t.view(c, b, h, w).permute(1, 0, 2, 3)


def backward_from_saved(gout: torch.Tensor, feat: torch.Tensor, acts: torch.Tensor,
                        params: Sequence[torch.Tensor], size: Sequence[int],
                        need_feat_grad: bool = True, head=None, chain=None) -> Tuple[Optional[torch.Tensor], List[torch.Tensor]]:
    """Gradients of the mode-3 decoder given d(loss)/d(out).

    gout [B,3,Hu,Wu]; feat [B,64,H,W]; acts [4,2,256,N] plain planes k_i, s_i (``untile_planes`` of the
    training forward's buffer, viewed [4,2,256,N]);
    params in PARAM_NAMES order.  Returns (d feat or None, [d param ...] in PARAM_NAMES order).

    With q_i = k_i * sin(s_i), k_0 = relu(P_0[cell]), k_i = relu(Wq_i q_{i-1} + P_i[cell]),
    s_0 = Q0 syn + bQ0, s_i = Qw_i q_{i-1} + bQ_i, out = L q_3 + bL:
        g_a,i = g_q,i * sin(s_i) * [k_i > 0]          g_s,i = g_q,i * k_i * cos(s_i)
        g_q,i-1 = Wq_i^T g_a,i + Qw_i^T g_s,i         dWq_i = g_a,i q_{i-1}^T   dQw_i = g_s,i q_{i-1}^T
        dP_i[cell] = sum over the cell's pixels of g_a,i;  P = conv3x3(feat; Wx) + bK.
    Computed in the dtype of ``acts`` (fp32 from the kernels; float64 planes give the formulas' own ground truth).
    ``head`` (decoder mode 4, mode4_training.backward_from_saved_mode4): (g_q,3 [256,N], d last_layer.weight, d last_layer.bias) of
    another head than the 1x1 one; ``params``' own ``last_layer`` tensors are then not read.
    ``chain`` (split_training.split_chain_backward_reference): a callable (Wq_i^T, g_a,i, Qw_i^T, g_s,i) -> g_q,i-1 that forms the
    chain product in another arithmetic; None: the two matrix products and their sum in ``acts``' dtype, as always."""
    dt = acts.dtype
    p = {name: t.to(dt) for name, t in zip(PARAM_NAMES, params)}
    feat = feat.to(dt)
    b, _, h, w = feat.shape
    hu, wu = int(size[0]), int(size[1])
    n = b * hu * wu
    dev = gout.device
    idx_h, rel_h, idx_w, rel_w, ratio = coordinate_tensors(h, w, hu, wu, dev)
    rel_h, rel_w = rel_h.to(dt), rel_w.to(dt)
    grads: Dict[str, torch.Tensor] = {}

    if head is not None:
        g_q, grads["last_layer.weight"], grads["last_layer.bias"] = head
    else:
        g_out = gout.to(dt).permute(1, 0, 2, 3).reshape(3, n)
        lw = p["last_layer.weight"].reshape(3, HIDDEN)
        q3 = acts[3, 0] * torch.sin(acts[3, 1])
        grads["last_layer.weight"] = (g_out @ q3.t()).reshape(3, HIDDEN, 1, 1)
        grads["last_layer.bias"] = g_out.sum(1)
        del q3
        g_q = lw.t() @ g_out                                      # [256, N]

    d_p: List[Optional[torch.Tensor]] = [None] * 4                # each [B,256,H,W]
    d_wq: List[Optional[torch.Tensor]] = [None] * 4
    for i in (3, 2, 1):
        k, s = acts[i, 0], acts[i, 1]
        g_a = g_q * torch.sin(s) * (k > 0)
        g_s = g_q * k * torch.cos(s)
        q_prev = acts[i - 1, 0] * torch.sin(acts[i - 1, 1])
        wfull = p[f"K.{i}.0.weight"].reshape(HIDDEN, HIDDEN + UNFOLD)
        qw = p[f"Q.{i}.0.weight"].reshape(HIDDEN, HIDDEN)
        d_wq[i] = g_a @ q_prev.t()
        grads[f"Q.{i}.0.weight"] = (g_s @ q_prev.t()).reshape(HIDDEN, HIDDEN, 1, 1)
        grads[f"Q.{i}.0.bias"] = g_s.sum(1)
        d_p[i] = _cell_sum(g_a, b, hu, wu, h, w, idx_h, idx_w)
        g_q = wfull[:, :HIDDEN].t() @ g_a + qw.t() @ g_s if chain is None else chain(wfull[:, :HIDDEN].t(), g_a, qw.t(), g_s)
        del g_a, g_s, q_prev
    k, s = acts[0, 0], acts[0, 1]
    g_a = g_q * torch.sin(s) * (k > 0)
    g_s = g_q * k * torch.cos(s)
    d_p[0] = _cell_sum(g_a, b, hu, wu, h, w, idx_h, idx_w)
    # syn = (rel_h, rel_w, ratio) per pixel (diinn.py:165-167): dQ0 = g_s syn^T without materialising syn
    g_s4 = g_s.view(HIDDEN, b, hu, wu)
    d_q0 = torch.stack([(g_s4.sum((1, 3)) * rel_h).sum(1), (g_s4.sum((1, 2)) * rel_w).sum(1),
                        g_s4.sum((1, 2, 3)) * ratio], dim=1)
    grads["Q.0.0.weight"] = d_q0.reshape(HIDDEN, 3, 1, 1)
    grads["Q.0.0.bias"] = g_s.sum(1)
    del g_a, g_s, g_q

    dp = torch.cat(d_p, dim=1).contiguous()                       # [B,1024,H,W]
    d_bk = dp.sum((0, 2, 3)).view(4, HIDDEN)
    wx = _hoisted_conv_weight(p)
    d_wx = torch.nn.grad.conv2d_weight(feat, wx.shape, dp, padding=1)
    d_feat = torch.nn.grad.conv2d_input(feat.shape, wx, dp, padding=1) if need_feat_grad else None
    _assemble_k_grads(grads, d_wx, d_wq, d_bk)
    return d_feat, [grads[name] for name in PARAM_NAMES]


WGRAD_CONV_KSPLIT = 12     # pixel-axis splits of the hoisted conv's weight-gradient GEMM (20 output blocks x 12)


def _conv_grads_native(feat: torch.Tensor, wx: torch.Tensor, dp: torch.Tensor, need_feat_grad: bool, want_weight: bool = True,
                       wkey=None, wpins=None, a_t: Optional[torch.Tensor] = None, rows: int = 4 * HIDDEN):
    """Gradients of P = conv3x3(feat; Wx[1024,64,3,3]) on the library's own kernels (no MIOpen in the decoder's step):
      weight:  dWx[o, (c,ky,kx)] = sum over cells of dP[o, cell] * unfold3x3(feat)[(c,ky,kx), cell] -- the plane GEMM over the
               cell axis (plane_gemm_lds_kernel; the 576 unfolded rows padded to 640 = 5 x 128);
      input :  d_feat = conv3x3(dP; Wx transposed and flipped) -- a 64-output 3x3 convolution over 1024 planes, i.e. the
               encoder's convolution kernels (Winograd F(4x4) / F(2x2) / split-K by the trunk's rule, convs.conv_form).
    ``rows`` < 1024 (decoder mode 1: 256, only P_0 is a convolution of the features): the conv is Wx[:rows], i.e. the first
    ``rows`` planes of ``dp`` [B,1024,H,W] / rows of ``a_t`` are used and ``wx`` is [rows,64,3,3].
    The weight and its cache key are the caller's: ``wx`` (a tensor, or a callable returning it, evaluated only when the
    transposed weight has to be repacked), ``wkey`` (what identifies its values: the DIINN callers pass their K weights'
    (address, version) pairs, MetaSR its own tagged tuple) and ``wpins`` (the tensors the key describes)."""
    b, c, h, w = feat.shape
    n = b * h * w
    dev = feat.device
    dp = dp.contiguous()
    d_wx = None
    if want_weight:
        # both operands as tiled plane groups over the CELL axis: dP from cell_sum_kernel itself (``a_t``: no transposing copy),
        # the reference's unfold (rows (c, ky, kx), diinn.py:168) from unfold_tiled_kernel (rows 576..639 zero)
        tiles = (n + PLANE_TILE - 1) // PLANE_TILE
        b_t = torch.empty((tiles, 640, PLANE_TILE), dtype=torch.float32, device=dev)
        if a_t is None:
            a_t = tile_planes(dp.permute(1, 0, 2, 3).reshape(4 * HIDDEN, n))
        # the product is taken transposed, dWx^T [640 x 1024] = unfold . dP^T: with 1024 = 4 x 256 columns it runs on the kernel's
        # 128 x 256 block form (113 TFLOP/s; the 128 x 128 form the 640 columns of dWx would need: 70)
        ks = max(1, min(WGRAD_CONV_KSPLIT, a_t.shape[0]))
        part = torch.empty((ks, 640, rows), dtype=torch.float32, device=dev)
    d_feat = None
    with _native.launcher(dev) as run:
        if want_weight:
            run("diinn_unfold_tiled", feat.contiguous(), b_t, 640, b, h, w)
            run("diinn_plane_gemm_nt", b_t, 640, 0, a_t, 4 * HIDDEN, 0, part, 640, rows, n, ks, 0)
            d_wx = _sum_parts(part.view(1, ks, -1)).view(640, rows)[:UNFOLD].t()
        if need_feat_grad:
            d_feat = torch.empty((b, c, h, w), dtype=torch.float32, device=dev)
            zero = torch.zeros(64, dtype=torch.float32, device=dev)
            cin, in_bs = rows, 4 * HIDDEN * h * w                # the planes convolved; the batch stride of dp
            form = convs.conv_form(b, h, w)
            # the transposed weight in the kernel's form: repacked only when a K weight changed (an optimizer step, a
            # load_state_dict), not on every backward call.  The Winograd transforms are taken in float64 and rounded once,
            # like the encoder's: F(4x4)'s gradient error 2.5e-5 -> ~1e-5 of max|d_feat| (the fixtures' bound is 1e-4).
            # One entry per (kernel form, device): a multi-scale step alternates forms without evicting each other.  An entry
            # PINS the weight tensors its key describes (as ``kept`` does): while it is cached their addresses cannot be
            # handed to another decoder's weights with equal version counts.
            key = (str(dev), wkey, rows)
            ent = _dgrad_pack.get((form, str(dev)))
            if wkey is None or ent is None or ent[0] != key:
                if callable(wx):                                 # (a caller whose weight is itself derived builds it only for a repack)
                    wx = wx()
                wt = wx.flip(2, 3).permute(1, 0, 2, 3).contiguous()      # [64, 1024, 3, 3]
                ent = (key, convs.pack_conv3x3(wt, form), tuple(t.detach() for t in (wpins or ())))
                if wkey is not None:
                    _dgrad_pack[(form, str(dev))] = ent
            # (F(4x4) takes the encoder's split area of this (device, stream): a partly filled last round is split over the input channels)
            ws = convs.w4_area(dev) if form == "wino4" else None
            convs.launch_conv3x3(form, run.stream, ws, b, h, w, dp, 0, in_bs, cin, ent[1], zero, None, 0, 0, d_feat, 0, c * h * w, 0)
    return d_wx, d_feat


_dgrad_pack: Dict[tuple, tuple] = {}               # (form, device) -> (key, the transposed hoisted-conv weight in that kernel's form, the pinned K weights)


def _assemble_k_grads(grads: Dict[str, torch.Tensor], d_wx: torch.Tensor, d_wq, d_bk) -> None:
    """The K.i gradients in the reference's [256, 256+576] layout: (dWq_i | layer i's rows of dWx); K.0 has no Wq."""
    d_wx = d_wx.reshape(4, HIDDEN, UNFOLD)
    grads["K.0.0.weight"] = d_wx[0].reshape(HIDDEN, UNFOLD, 1, 1)
    grads["K.0.0.bias"] = d_bk[0]
    for i in (1, 2, 3):
        grads[f"K.{i}.0.weight"] = torch.cat([d_wq[i], d_wx[i]], dim=1).reshape(HIDDEN, HIDDEN + UNFOLD, 1, 1)
        grads[f"K.{i}.0.bias"] = d_bk[i]


PLANE_TILE = 32


def tile_planes(x: torch.Tensor) -> torch.Tensor:
    """Plain planes [C, n] -> tiled group [ceil(n/32), C, 32] (zero padding), the layout of include/diinn_hip.h."""
    c, n = x.shape
    t = (n + PLANE_TILE - 1) // PLANE_TILE
    out = x.new_zeros((c, t * PLANE_TILE))
    out[:, :n] = x
    return out.view(c, t, PLANE_TILE).permute(1, 0, 2).contiguous()


def untile_planes(x: torch.Tensor, n: int) -> torch.Tensor:
    """Tiled groups [..., T, C, 32] -> plain planes [..., C, n] (a copy; tests and the formula path)."""
    *lead, t, c, w = x.shape
    d = len(lead)
    return x.permute(*range(d), d + 1, d, d + 2).reshape(*lead, c, t * w)[..., :n]


_geometry_cache: "Dict[tuple, dict]" = {}


def _geometry(b: int, h: int, w: int, hu: int, wu: int, dev) -> dict:
    """Per-shape constants of the backward pass, built once per (B, LR size, HR size, device): the cell
    rectangles of cell_sum_kernel and the tiled right-hand side (rel_h, rel_w, ratio, 1) of the layer-0
    product.  Training revisits a handful of shapes (one per scale), so a small LRU suffices."""
    def build():
        idx_h, rel_h, idx_w, rel_w, ratio = coordinate_tensors(h, w, hu, wu, dev)
        syn = torch.empty((4, b, hu, wu), dtype=torch.float32, device=dev)
        syn[0] = rel_h[None, :, None]
        syn[1] = rel_w[None, None, :]
        syn[2] = ratio
        syn[3] = 1.0
        return {
            "seg_h": torch.searchsorted(idx_h, torch.arange(h + 1, device=dev)).to(torch.int32),
            "seg_w": torch.searchsorted(idx_w, torch.arange(w + 1, device=dev)).to(torch.int32),
            "syn_t": tile_planes(syn.view(4, b * hu * wu)),
        }
    return lru(_geometry_cache, (b, h, w, hu, wu, str(dev)), build)


def _sum_parts(part: torch.Tensor) -> torch.Tensor:
    """[groups, nparts, n] -> [groups, n]: the split partials of a GEMM / rowdot launch added in slice order (sum_parts_kernel)."""
    groups, nparts, n = part.shape
    if n % 4 or not part.is_contiguous():
        return part.sum(1)
    out = torch.empty((groups, n), dtype=torch.float32, device=part.device)
    with _native.launcher(part.device) as run:
        run("diinn_sum_parts", part, out, groups, nparts, n)
    return out


class ChainPlanes:
    """The prologue of every per-pixel backward: the shape numbers (b, h, w, hu, wu, n = B*Hu*Wu, t tiles, dev), the check of
    ``acts``, g_out as planes ``gp`` [3, N] and the empty tiled groups the data kernel fills, ``g`` [4,T,512,32] and ``q`` [4,T,256,32]."""

    def __init__(self, gout: torch.Tensor, feat: torch.Tensor, acts: torch.Tensor, size: Sequence[int]):
        self.b, _, self.h, self.w = feat.shape
        self.hu, self.wu = int(size[0]), int(size[1])
        self.n = n = self.b * self.hu * self.wu
        self.t = t = (n + PLANE_TILE - 1) // PLANE_TILE
        self.dev = dev = gout.device
        if tuple(acts.shape) != (4, t, 2 * HIDDEN, PLANE_TILE) or not acts.is_contiguous():
            raise ValueError("acts must be the contiguous tiled [4, T, 512, 32] buffer of the training forward")
        self.gp = gout.to(torch.float32).permute(1, 0, 2, 3).reshape(3, n).contiguous()
        self.g = torch.empty((4, t, 2 * HIDDEN, PLANE_TILE), dtype=torch.float32, device=dev)
        self.q = torch.empty((4, t, HIDDEN, PLANE_TILE), dtype=torch.float32, device=dev)


def head_rhs(gp: torch.Tensor) -> torch.Tensor:
    """(g_out ; 0) tiled: the 4-row right-hand side of the 1x1 head's product."""
    return tile_planes(torch.cat([gp, gp.new_zeros((1, gp.shape[1]))], 0))


class ChainStage(ChainPlanes):
    """The per-pixel chain of a backward pass, stated once for ``backward_fused`` and ``initq_training.backward_fused_initq``.

    ``ChainStage(...)``  the checks and the buffers (``ChainPlanes``; ``geo``: ``_geometry``; the splits; the partials ``part``,
                         ``part0``, ``partl``), before any launch
    ``launch(run)``      on the caller's ``run`` (_native.launcher), whose own launches follow in the same block:
      the data kernel       diinn_backward_data, or _x3 (``split``: the split training image), _head3x3 (``head``: the 3x3 head image;
                            it also writes dT as seven 4-row groups, row 27 zero) or _qonly followed by diinn_pixel_chain_bwd
                            (``qonly``): leaves G_i = (g_a,i ; g_s,i) in ``g`` and q_i in ``q`` as tiled planes
      diinn_plane_gemm_nt   [dWq_i ; dQw_i | bias sums] = G_i [512 x N] . q_{i-1}^T, i = 3, 2, 1 (``qonly``: two 256-row products per
                            layer, [dKk_i | dbK_i] = g_a,i . k_{i-1}^T on the saved k planes, then [dQw_i | dbQ_i] = g_s,i . q_{i-1}^T)
      diinn_plane_rowdot    G_0 against (rel_h, rel_w, ratio, 1); q_3 against each 4-row group of the head's right-hand side
    ``grads(grads)``     the sums of the head's and the layers' partials as gradients; ``layer0()`` those of the layer-0 product."""

    def __init__(self, gout: torch.Tensor, feat: torch.Tensor, acts: torch.Tensor, packed: torch.Tensor, size: Sequence[int],
                 head: Optional[torch.Tensor] = None, split: Optional[torch.Tensor] = None, qonly: bool = False):
        super().__init__(gout, feat, acts, size)
        if qonly and head is not None:
            raise ValueError("qonly (modes 1/2) and head (mode 4) exclude each other")
        self.acts, self.packed, self.head, self.split, self.qonly = acts, packed, head, split, qonly
        n, t = self.n, self.t
        f32 = dict(dtype=torch.float32, device=self.dev)
        self.geo = _geometry(self.b, self.h, self.w, self.hu, self.wu, self.dev)
        if head is None:
            self.heads = head_rhs(self.gp)[None]
        else:
            # the rowdot reads whole tiles: a ragged last tile's padding is zeroed here
            self.heads = (torch.empty if n % PLANE_TILE == 0 else torch.zeros)((7, t, 4, PLANE_TILE), **f32)
        # (qonly: the weight-gradient GEMMs have 256 rows = 2 output blocks; twice the splits make one workgroup per CU, as in backward_fused_modes12)
        self.ksplit = max(1, min(2 * WGRAD_KSPLIT if qonly else WGRAD_KSPLIT, t))
        self.rsplit = max(1, min(ROWDOT_SPLITS, t))
        self.part = torch.empty((6, self.ksplit, HIDDEN, HIDDEN + 1) if qonly else (3, self.ksplit, 2 * HIDDEN, HIDDEN + 1), **f32)
        self.part0 = torch.empty((self.rsplit, 2 * HIDDEN, 4), **f32)
        self.partl = torch.empty((len(self.heads), self.rsplit, HIDDEN, 4), **f32)

    def launch(self, run) -> None:
        gp, acts, packed, g, q, part, n, ksplit = self.gp, self.acts, self.packed, self.g, self.q, self.part, self.n, self.ksplit
        if self.qonly:
            run("diinn_backward_data_qonly", gp, acts, packed, g, q, n)
            run("diinn_pixel_chain_bwd", g, acts, packed, n)
            for i in (3, 2, 1):
                run("diinn_plane_gemm_nt", g[i], 2 * HIDDEN, 0, acts[i - 1], 2 * HIDDEN, 0, part[2 * (i - 1)], HIDDEN, HIDDEN, n, ksplit, 1)
                run("diinn_plane_gemm_nt", g[i], 2 * HIDDEN, HIDDEN, q[i - 1], HIDDEN, 0, part[2 * (i - 1) + 1], HIDDEN, HIDDEN, n, ksplit, 1)
        else:
            if self.split is not None:
                run("diinn_backward_data_x3", gp, acts, packed, self.split, g, q, n)
            elif self.head is None:
                run("diinn_backward_data", gp, acts, packed, g, q, n)
            else:
                run("diinn_backward_data_head3x3", gp, acts, packed, self.head, g, q, self.heads, self.b, self.hu, self.wu)
            for i in (3, 2, 1):
                run("diinn_plane_gemm_nt", g[i], 2 * HIDDEN, 0, q[i - 1], HIDDEN, 0, part[i - 1], 2 * HIDDEN, HIDDEN, n, ksplit, 1)
        run("diinn_plane_rowdot", g[0], 2 * HIDDEN, self.geo["syn_t"], self.part0, 2 * HIDDEN, n, self.rsplit)
        for i in range(len(self.heads)):
            run("diinn_plane_rowdot", q[3], HIDDEN, self.heads[i], self.partl[i], HIDDEN, n, self.rsplit)

    def grads(self, grads: Dict[str, torch.Tensor]):
        """``last_layer.*`` and ``Q.i.*`` (i = 3, 2, 1) into ``grads``; returns (dWq, dbK), lists whose entries 1..3 are dWq_i [256,256]
        and dbK_i [256] (entry 0 None: layer 0 is the caller's)."""
        groups = len(self.heads)
        dl = _sum_parts(self.partl.view(groups, self.rsplit, -1)).view(groups, HIDDEN, 4)    # group i: q_3 . (rows 4 i .. 4 i + 3 of the right-hand side)^T
        if self.head is None:
            head1x1_grads(grads, dl[0], self.gp)
        else:                                                    # [256, r = 3 (3 ky + kx) + c] -> [c, ch, ky, kx]
            grads["last_layer.weight"] = dl.permute(1, 0, 2).reshape(HIDDEN, 28)[:, :27].t().reshape(3, 3, 3, HIDDEN).permute(2, 3, 0, 1).contiguous()
            grads["last_layer.bias"] = self.gp.sum(1)
        # [3, 512, 257]: [dWq_i ; dQw_i | bias sums] (qonly: the two 256-row products of a layer are neighbours in ``part``: the same view)
        dws = _sum_parts(self.part.view(self.part.shape[0], self.ksplit, -1)).view(3, 2 * HIDDEN, HIDDEN + 1)
        d_wq: List[Optional[torch.Tensor]] = [None] * 4
        d_bk: List[Optional[torch.Tensor]] = [None] * 4
        for i in (3, 2, 1):
            dw = dws[i - 1]
            d_wq[i] = dw[:HIDDEN, :HIDDEN]
            d_bk[i] = dw[:HIDDEN, HIDDEN]
            grads[f"Q.{i}.0.weight"] = dw[HIDDEN:, :HIDDEN].reshape(HIDDEN, HIDDEN, 1, 1)
            grads[f"Q.{i}.0.bias"] = dw[HIDDEN:, HIDDEN]
        return d_wq, d_bk

    def layer0(self) -> torch.Tensor:
        """[512, 4]: (g_a,0 ; g_s,0) . (rel_h, rel_w, ratio, 1)^T -- column 3 is (dbK_0 ; dbQ_0)."""
        return _sum_parts(self.part0.view(1, self.rsplit, -1)).view(2 * HIDDEN, 4)


def head1x1_grads(grads: Dict[str, torch.Tensor], dl: torch.Tensor, gp: torch.Tensor) -> None:
    """d last_layer.* of the 1x1 head from ``dl`` [256, 4] = q_3 . (g_out ; 0)^T and the planes of g_out."""
    grads["last_layer.weight"] = dl[:, :3].t().reshape(3, HIDDEN, 1, 1)
    grads["last_layer.bias"] = gp.sum(1)


def backward_fused(gout: torch.Tensor, feat: torch.Tensor, acts: torch.Tensor, params: Sequence[torch.Tensor],
                   packed: torch.Tensor, size: Sequence[int],
                   need_feat_grad: bool = True, head: Optional[torch.Tensor] = None, split: Optional[torch.Tensor] = None
                   ) -> Tuple[Optional[torch.Tensor], List[torch.Tensor]]:
    """The same gradients as ``backward_from_saved``, on the HIP kernels throughout:
      diinn_backward_data   3 x bwd_layer_kernel (the head's gates inside layer 3's): the per-pixel chain; leaves the
                            gate gradients G_i = (g_a,i ; g_s,i) and the activations q_i as tiled planes
      diinn_plane_gemm_nt   [dWq_i ; dQw_i | bias sums] = G_i [512 x N] . q_{i-1}^T [N x 256], split over pixels
      diinn_plane_rowdot    the two skinny products (layer 0 against (rel_h, rel_w, ratio, 1); head against g_out)
      diinn_backward_cell_sum   dP = per-cell sums of g_a, NCHW and tiled over the cell axis
      _conv_grads_native    the 3x3 convolution's weight gradient (unfold + plane GEMM) and input gradient (encoder conv kernels)
    ``acts`` is the tiled buffer [4, T, 512, 32] of the training forward.
    ``head`` (decoder mode 4): the 3x3 head image (mode4_training.pack_head3x3_on_device); ``packed`` is then the body image with a
    zero 1x1 head.  Three things change, the rest is the same code: the chain starts with diinn_backward_data_head3x3 (the head's
    adjoint dT and layer 3's gates in bwd_head3x3_kernel, then layers 3, 2, 1); d last_layer.weight [3,256,3,3] is q_3 against the
    seven 4-row groups of dT (7 x diinn_plane_rowdot, diinn_sum_parts); d last_layer.bias is the sum of g as before.
    ``split`` (mode 3 only; split_training.pack_split_on_device): the split training image -- the chain then runs on
    diinn_backward_data_x3 (3 x bwd_layer_x3_kernel, split-bf16 arithmetic) in place of diinn_backward_data; the planes it leaves
    have the same layout and everything behind them is the same code.  None: today's fp32 chain."""
    if split is not None and head is not None:
        raise ValueError("the split-bf16 chain covers mode 3 only (no 3x3 head)")
    p = dict(zip(PARAM_NAMES, params))
    c = ChainStage(gout, feat, acts, packed, size, head=head, split=split)
    b, h, w, dev = c.b, c.h, c.w, c.dev
    dp = torch.empty((b, 4 * HIDDEN, h, w), dtype=torch.float32, device=dev)
    # the hoisted conv's weight gradient on the library's own GEMM wants dP tiled over the cell axis as well: cell_sum_kernel
    # writes it (a ragged last tile's padding must be zero: the GEMM reads whole tiles)
    cells = b * h * w
    a_t = (torch.empty if cells % PLANE_TILE == 0 else torch.zeros)(((cells + PLANE_TILE - 1) // PLANE_TILE, 4 * HIDDEN, PLANE_TILE),
                                                                    dtype=torch.float32, device=dev)
    with _native.launcher(dev) as run:
        c.launch(run)
        run("diinn_backward_cell_sum", c.g, c.geo["seg_h"], c.geo["seg_w"], dp, a_t, b, h, w, c.hu, c.wu)
    grads: Dict[str, torch.Tensor] = {}
    d_wq, d_bk = c.grads(grads)
    d0 = c.layer0()
    d_bk[0] = d0[:HIDDEN, 3]
    grads["Q.0.0.weight"] = d0[HIDDEN:, :3].reshape(HIDDEN, 3, 1, 1)
    grads["Q.0.0.bias"] = d0[HIDDEN:, 3]
    kw = tuple(p[f"K.{i}.0.weight"] for i in range(4))
    d_wx, d_feat = _conv_grads_native(feat, _hoisted_conv_weight(p), dp, need_feat_grad, wkey=weights_key(kw), wpins=kw, a_t=a_t)
    _assemble_k_grads(grads, d_wx, d_wq, d_bk)
    return d_feat, [grads[name] for name in PARAM_NAMES]


# ---------------------------------------------------------------------------
# decoder modes 1 and 2 (diinn.py:116-131): the modulation chain lives on the LR cells
# ---------------------------------------------------------------------------
def cell_chain_planes(feat: torch.Tensor, params: Sequence[torch.Tensor], mode: int) -> torch.Tensor:
    """k_i per LR cell, [4, 256, B*H*W] (cell index (b*H + cy)*W + cx), in plain tensor algebra:
    k_0 = relu(P_0), k_i = relu(Kk_i k_{i-1} + P_i) with P = conv3x3(feat; Wx) + bK (mode 1: P_i = bK_i for i >= 1)."""
    p = dict(zip(PARAM_NAMES, params))
    b, _, h, w = feat.shape
    cells = b * h * w
    wx = _hoisted_conv_weight(p, mode)
    conv = torch.nn.functional.conv2d(feat, wx, padding=1).permute(1, 0, 2, 3).reshape(-1, cells)     # [1024 or 256, cells]
    ks = []
    k = None
    for i in range(4):
        a = p[f"K.{i}.0.bias"].reshape(HIDDEN, 1).expand(HIDDEN, cells)
        if i == 0 or mode != 1:
            a = a + conv[i * HIDDEN:(i + 1) * HIDDEN]
        if i:
            a = a + p[f"K.{i}.0.weight"].reshape(HIDDEN, -1)[:, :HIDDEN] @ k
        k = torch.relu(a)
        ks.append(k)
    return torch.stack(ks)


def backward_from_saved_modes12(gout: torch.Tensor, feat: torch.Tensor, acts: torch.Tensor,
                                params: Sequence[torch.Tensor], size: Sequence[int], mode: int,
                                need_feat_grad: bool = True, cell_k: Optional[torch.Tensor] = None
                                ) -> Tuple[Optional[torch.Tensor], List[torch.Tensor]]:
    """Gradients of the mode-1 / mode-2 decoder given d(loss)/d(out): ``backward_from_saved``'s counterpart.

    acts [4,2,256,N]: k_i of the pixel's cell (replicated per pixel) and s_i; params in PARAM_NAMES order with ``mode``'s shapes;
    cell_k [4,256,B*H*W]: k_i per LR cell (``cell_chain_planes``; recomputed from feat when None -- a cell that owns no
    HR pixel does not appear in ``acts``).

    With q_i = k_i[cell] * sin(s_i), s_0 = Q0 syn + bQ0, s_i = Qw_i q_{i-1} + bQ_i, k_0 = relu(P_0), k_i = relu(Kk_i k_{i-1} + P_i),
    Kk_i = K.i.weight[:, :256], out = L q_3 + bL (diinn.py:116-131), per HR pixel (i = 3..0)
        g_s,i = g_q,i * k_i * cos(s_i)        g^_a,i = g_q,i * sin(s_i) * [k_i > 0]        g_q,i-1 = Qw_i^T g_s,i   (no Wq^T g_a term)
        dQw_i = g_s,i q_{i-1}^T               dbQ_i = sum over pixels of g_s,i
    and per LR cell, with S_i = sum over the cell's pixels of g^_a,i:
        g_a,3 = S_3        g_a,i-1 = [k_{i-1} > 0] * (Kk_i^T g_a,i) + S_{i-1}        dP_i = g_a,i
        dKk_i = sum over cells of g_a,i k_{i-1}^T        dbK_i = sum over CELLS of g_a,i   (not the pixel sum of g^_a,i)
    The conv's gradients come from dP: all 1024 rows in mode 2, layer 0's 256 rows in mode 1."""
    if mode not in (1, 2):
        raise ValueError("backward_from_saved_modes12 covers decoder modes 1 and 2")
    p = dict(zip(PARAM_NAMES, params))
    b, _, h, w = feat.shape
    hu, wu = int(size[0]), int(size[1])
    n = b * hu * wu
    cells = b * h * w
    dev = gout.device
    idx_h, rel_h, idx_w, rel_w, ratio = coordinate_tensors(h, w, hu, wu, dev)
    if cell_k is None:
        cell_k = cell_chain_planes(feat, params, mode)
    grads: Dict[str, torch.Tensor] = {}

    g_out = gout.to(torch.float32).permute(1, 0, 2, 3).reshape(3, n)
    lw = p["last_layer.weight"].reshape(3, HIDDEN)
    q3 = acts[3, 0] * torch.sin(acts[3, 1])
    grads["last_layer.weight"] = (g_out @ q3.t()).reshape(3, HIDDEN, 1, 1)
    grads["last_layer.bias"] = g_out.sum(1)
    del q3
    g_q = lw.t() @ g_out                                          # [256, N]

    s_cell: List[Optional[torch.Tensor]] = [None] * 4             # each [256, cells]
    for i in (3, 2, 1, 0):
        k, s = acts[i, 0], acts[i, 1]
        g_a = g_q * torch.sin(s) * (k > 0)
        g_s = g_q * k * torch.cos(s)
        s_cell[i] = _cell_sum(g_a, b, hu, wu, h, w, idx_h, idx_w).permute(1, 0, 2, 3).reshape(HIDDEN, cells)
        if i:
            q_prev = acts[i - 1, 0] * torch.sin(acts[i - 1, 1])
            grads[f"Q.{i}.0.weight"] = (g_s @ q_prev.t()).reshape(HIDDEN, HIDDEN, 1, 1)
            grads[f"Q.{i}.0.bias"] = g_s.sum(1)
            g_q = p[f"Q.{i}.0.weight"].reshape(HIDDEN, HIDDEN).t() @ g_s
        else:
            # syn = (rel_h, rel_w, ratio) per pixel (diinn.py:165-167): dQ0 = g_s syn^T without materialising syn
            g_s4 = g_s.view(HIDDEN, b, hu, wu)
            d_q0 = torch.stack([(g_s4.sum((1, 3)) * rel_h).sum(1), (g_s4.sum((1, 2)) * rel_w).sum(1),
                                g_s4.sum((1, 2, 3)) * ratio], dim=1)
            grads["Q.0.0.weight"] = d_q0.reshape(HIDDEN, 3, 1, 1)
            grads["Q.0.0.bias"] = g_s.sum(1)
    del g_a, g_s, g_q

    d_p: List[Optional[torch.Tensor]] = [None] * 4                # each [256, cells]
    d_kk: List[Optional[torch.Tensor]] = [None] * 4
    g_a = s_cell[3]
    d_p[3] = g_a
    for i in (3, 2, 1):
        kk = p[f"K.{i}.0.weight"].reshape(HIDDEN, -1)[:, :HIDDEN]
        d_kk[i] = g_a @ cell_k[i - 1].t()
        g_a = (cell_k[i - 1] > 0) * (kk.t() @ g_a) + s_cell[i - 1]
        d_p[i - 1] = g_a
    dp = torch.stack(d_p).view(4 * HIDDEN, b, h, w).permute(1, 0, 2, 3).contiguous()        # [B,1024,H,W]
    d_bk = dp.sum((0, 2, 3)).view(4, HIDDEN)
    wx = _hoisted_conv_weight(p, mode)
    dpc = dp[:, :wx.shape[0]].contiguous()
    d_wx = torch.nn.grad.conv2d_weight(feat, wx.shape, dpc, padding=1)
    d_feat = torch.nn.grad.conv2d_input(feat.shape, wx, dpc, padding=1) if need_feat_grad else None
    _assemble_k_grads_modes12(grads, d_wx, d_kk, d_bk, mode)
    return d_feat, [grads[name] for name in PARAM_NAMES]


def _assemble_k_grads_modes12(grads: Dict[str, torch.Tensor], d_wx: torch.Tensor, d_kk, d_bk, mode: int) -> None:
    """The K.i gradients in the reference's layout: mode 2 (dKk_i | layer i's rows of dWx) [256,832]; mode 1 dKk_i [256,256]."""
    d_wx = d_wx.reshape(-1, HIDDEN, UNFOLD)
    grads["K.0.0.weight"] = d_wx[0].reshape(HIDDEN, UNFOLD, 1, 1)
    grads["K.0.0.bias"] = d_bk[0]
    for i in (1, 2, 3):
        if mode == 1:
            grads[f"K.{i}.0.weight"] = d_kk[i].reshape(HIDDEN, HIDDEN, 1, 1)
        else:
            grads[f"K.{i}.0.weight"] = torch.cat([d_kk[i], d_wx[i]], dim=1).reshape(HIDDEN, HIDDEN + UNFOLD, 1, 1)
        grads[f"K.{i}.0.bias"] = d_bk[i]


_cell_ones_cache: Dict[tuple, torch.Tensor] = {}


def _cell_ones(cells: int, dev) -> torch.Tensor:
    """The tiled 4-row group of ones over ``cells`` cells (zero padding): diinn_plane_rowdot against it sums dP over the cells.
    Kept per (cell count, device) like the geometry constants (one entry per batch geometry of a training run)."""
    return lru(_cell_ones_cache, (cells, str(dev)), lambda: tile_planes(torch.ones((4, cells), dtype=torch.float32, device=dev)))


def backward_fused_modes12(gout: torch.Tensor, feat: torch.Tensor, acts: torch.Tensor, chain: torch.Tensor,
                           params: Sequence[torch.Tensor], packed: torch.Tensor, size: Sequence[int], mode: int,
                           need_feat_grad: bool = True) -> Tuple[Optional[torch.Tensor], List[torch.Tensor]]:
    """The same gradients as ``backward_from_saved_modes12``, on the HIP kernels throughout:
      diinn_backward_data_qonly  3 x bwd_layer_kernel<., KPART=false>: g_q,i-1 = Qw_i^T g_s,i; leaves G_i = (g^_a,i ; g_s,i) and q_i
      diinn_plane_gemm_nt        [dQw_i | dbQ_i] = g_s,i [256 x N] . q_{i-1}^T, split over pixels
      diinn_plane_rowdot         g_s,0 against (rel_h, rel_w, ratio, 1); the head against g_out
      diinn_backward_cell_sum    S = per-cell sums of g^_a, tiled over the cell axis
      diinn_cell_chain_bwd       the chain backwards: dP (in place of S, and NCHW) and k_0..k_2 tiled over cells
      diinn_plane_gemm_nt        dKk_i = dP_i [256 x cells] . k_{i-1}^T;  diinn_plane_rowdot against ones: dbK = sum of dP over cells
      _conv_grads_native         the 3x3 convolution's gradients from dP (mode 1: layer 0's 256 rows)
    ``acts`` is the tiled buffer [4, T, 512, 32] of the training forward, ``chain`` its [B,H,W,1024] workspace.
    Of ``ChainStage`` this shares the prologue (``ChainPlanes``) and the 1x1 head; its GEMMs take the lower 256 rows of G_i alone and
    its layer-0 product the lower half-plane."""
    if mode not in (1, 2):
        raise ValueError("backward_fused_modes12 covers decoder modes 1 and 2")
    p = dict(zip(PARAM_NAMES, params))
    c = ChainPlanes(gout, feat, acts, size)
    b, h, w, hu, wu, n, t, dev, gp, g, q = c.b, c.h, c.w, c.hu, c.wu, c.n, c.t, c.dev, c.gp, c.g, c.q
    cells = b * h * w
    tc = (cells + PLANE_TILE - 1) // PLANE_TILE
    if chain.numel() != cells * 4 * HIDDEN or not chain.is_contiguous():
        raise ValueError("chain must be the contiguous [B,H,W,1024] workspace of the training forward")
    geo = _geometry(b, h, w, hu, wu, dev)
    ones_t = _cell_ones(cells, dev)
    gout_t = head_rhs(gp)
    f32 = dict(dtype=torch.float32, device=dev)
    # the weight-gradient GEMMs here have 256 rows = 2 output blocks (mode 3's: 512 rows = 4): twice the splits make one workgroup per CU
    ksplit = max(1, min(2 * WGRAD_KSPLIT, t))
    kcsplit = max(1, min(2 * WGRAD_KSPLIT, tc))
    rsplit = max(1, min(ROWDOT_SPLITS, t))
    rcsplit = max(1, min(ROWDOT_SPLITS, tc))
    part = torch.empty((3, ksplit, HIDDEN, HIDDEN + 1), **f32)
    partk = torch.empty((3, kcsplit, HIDDEN, HIDDEN), **f32)
    part0 = torch.empty((rsplit, HIDDEN, 4), **f32)
    partl = torch.empty((rsplit, HIDDEN, 4), **f32)
    partb = torch.empty((2, rcsplit, 2 * HIDDEN, 4), **f32)
    dp = torch.empty((b, 4 * HIDDEN, h, w), **f32)
    alloc = torch.empty if cells % PLANE_TILE == 0 else torch.zeros      # (a ragged last tile's padding stays zero)
    a_t = alloc((tc, 4 * HIDDEN, PLANE_TILE), **f32)
    k_t = alloc((tc, 3 * HIDDEN, PLANE_TILE), **f32)
    with _native.launcher(dev) as run:
        run("diinn_backward_data_qonly", gp, acts, packed, g, q, n)
        for i in (3, 2, 1):
            run("diinn_plane_gemm_nt", g[i], 2 * HIDDEN, HIDDEN, q[i - 1], HIDDEN, 0, part[i - 1], HIDDEN, HIDDEN, n, ksplit, 1)
        # layer 0: only g_s,0 (rows 256..511 of G_0) meets (rel_h, rel_w, ratio, 1); dbK_0 comes from the chain below
        run("diinn_plane_rowdot", (g[0], HIDDEN * PLANE_TILE), 2 * HIDDEN, geo["syn_t"], part0, HIDDEN, n, rsplit)
        run("diinn_plane_rowdot", q[3], HIDDEN, gout_t, partl, HIDDEN, n, rsplit)
        run("diinn_backward_cell_sum", g, geo["seg_h"], geo["seg_w"], dp, a_t, b, h, w, hu, wu)
        run("diinn_cell_chain_bwd", a_t, chain, packed, dp, a_t, k_t, b, h, w)
        for i in (3, 2, 1):
            run("diinn_plane_gemm_nt", a_t, 4 * HIDDEN, i * HIDDEN, k_t, 3 * HIDDEN, (i - 1) * HIDDEN, partk[i - 1], HIDDEN, HIDDEN, cells, kcsplit, 0)
        for hf in (0, 1):                                        # rows 0..511 and 512..1023 of dP (of a tile of a_t) against ones
            run("diinn_plane_rowdot", (a_t, hf * 2 * HIDDEN * PLANE_TILE), 4 * HIDDEN, ones_t, partb[hf], 2 * HIDDEN, cells, rcsplit)
    grads: Dict[str, torch.Tensor] = {}
    head1x1_grads(grads, _sum_parts(partl.view(1, rsplit, -1)).view(HIDDEN, 4), gp)     # [256, 4]: q_3 . (g_out ; 0)^T
    dws = _sum_parts(part.view(3, ksplit, -1)).view(3, HIDDEN, HIDDEN + 1)        # [3, 256, 257]: [dQw_i | dbQ_i]
    dks = _sum_parts(partk.view(3, kcsplit, -1)).view(3, HIDDEN, HIDDEN)          # [3, 256, 256]: dKk_i
    d_bk = _sum_parts(partb.view(2, rcsplit, -1)).view(4, HIDDEN, 4)[:, :, 0]     # [4, 256]: sum of dP_i over the cells
    d_kk: List[Optional[torch.Tensor]] = [None] * 4
    for i in (3, 2, 1):
        d_kk[i] = dks[i - 1]
        grads[f"Q.{i}.0.weight"] = dws[i - 1][:, :HIDDEN].reshape(HIDDEN, HIDDEN, 1, 1)
        grads[f"Q.{i}.0.bias"] = dws[i - 1][:, HIDDEN]
    d0 = _sum_parts(part0.view(1, rsplit, -1)).view(HIDDEN, 4)    # [256, 4]: g_s,0 . (rel_h, rel_w, ratio, 1)^T
    grads["Q.0.0.weight"] = d0[:, :3].reshape(HIDDEN, 3, 1, 1)
    grads["Q.0.0.bias"] = d0[:, 3]
    kw = tuple(p[f"K.{i}.0.weight"] for i in range(4))
    wx = _hoisted_conv_weight(p, mode)
    d_wx, d_feat = _conv_grads_native(feat, wx, dp, need_feat_grad, wkey=(mode, *weights_key(kw)), wpins=kw, a_t=a_t, rows=wx.shape[0])
    _assemble_k_grads_modes12(grads, d_wx, d_kk, d_bk, mode)
    return d_feat, [grads[name] for name in PARAM_NAMES]


# ---------------------------------------------------------------------------
# autograd functions
# ---------------------------------------------------------------------------
def checked_features(feat: torch.Tensor, params: Sequence[torch.Tensor], names: Sequence[str], shapes: Dict[str, Tuple[int, ...]],
                     hu: int, wu: int, plane_rows: int, what: str = "") -> torch.Tensor:
    """The entry check of the training Functions (decoder modes 1-3, MetaSR): ``feat`` on a GPU, ``params`` the tensors ``names`` with
    ``shapes`` (``what`` completes the message), ``feat`` [B,64,H,W], B*Hu*Wu HR pixels within the limit of ``plane_rows``-row tiled
    planes.  Returns ``feat`` detached, contiguous, fp32."""
    if not feat.is_cuda:
        raise RuntimeError("diinn_amd: the training forward runs on a ROCm GPU only (no CPU implementation)")
    if len(params) != len(names):
        raise ValueError(f"expected {len(names)} parameter tensors in PARAM_NAMES order")
    for name, p_ in zip(names, params):
        if tuple(p_.shape) != shapes[name]:
            raise ValueError(f"{name}: expected shape {shapes[name]}{what}, got {tuple(p_.shape)}")
    feat_c = feat.detach().contiguous().to(torch.float32)
    if feat_c.dim() != 4 or feat_c.shape[1] != IN_CHANNELS:
        raise ValueError(f"feat must be [B,{IN_CHANNELS},H,W]")
    n = feat_c.shape[0] * hu * wu
    if _native.load().diinn_training_plane_floats(n, plane_rows) < 0:
        raise RuntimeError(f"diinn_amd: B*Hu*Wu = {n} HR pixels in one training forward exceeds the limit; split the batch")
    return feat_c


def named_params(module, names: Sequence[str]) -> List[torch.Tensor]:
    """``module``'s parameters ``names``, in that order: what a ``decode_with_grad`` hands its Function."""
    named = dict(module.named_parameters())
    return [named[name] for name in names]


def function_grads(ctx, d_feat: Optional[torch.Tensor], d_params: Sequence[Optional[torch.Tensor]], first: int) -> tuple:
    """What a training Function's ``backward`` returns: d feat, None for the integers behind it, and from input ``first`` on each
    parameter's gradient where one was asked for."""
    need = ctx.needs_input_grad[first:]
    return (d_feat, *[None] * (first - 1), *[g if nd else None for g, nd in zip(d_params, need)])


def train_buffers(feat_c: torch.Tensor, hu: int, wu: int, workspace=None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(acts [4,T,512,32], out [B,3,Hu,Wu], workspace) of a training forward on ``feat_c``: empty fp32 buffers on its device.
    ``workspace``: its float count; None: the hoisted conv's [B,H,W,1024]."""
    b, _, h, w = feat_c.shape
    f32 = dict(dtype=torch.float32, device=feat_c.device)
    acts = torch.empty((4, (b * hu * wu + PLANE_TILE - 1) // PLANE_TILE, 2 * HIDDEN, PLANE_TILE), **f32)
    return acts, torch.empty((b, 3, hu, wu), **f32), torch.empty((b, h, w, 4 * HIDDEN) if workspace is None else workspace, **f32)


def train_forward_mode3(feat_c: torch.Tensor, packed: torch.Tensor, hu: int, wu: int, sin_mode: int,
                        split: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The mode-3 training forward on a contiguous fp32 CUDA ``feat_c`` and its packed image: the hoisted conv on the Winograd
    kernel (diinn_precompute_P_wpu; the image carries its section, DIINN_PACKED_MAGIC_WPU: ``_fill_wpu``), then decode_kernel<SAVE>
    (diinn_decode_train_fwd) or, with the split training image ``split``, decode_bf16x3_kernel<SIN | X3_SAVE>
    (diinn_decode_train_fwd_x3).  Returns (out, acts [4,T,512,32])."""
    b, _, h, w = feat_c.shape
    acts, out, workspace = train_buffers(feat_c, hu, wu)
    with _native.launcher(feat_c.device) as run:
        run("diinn_precompute_P_wpu", feat_c, packed, workspace, b, h, w, 0, h)
        if split is None:
            run("diinn_decode_train_fwd", workspace, packed, out, acts, b, h, w, hu, wu, int(sin_mode))
        else:
            run("diinn_decode_train_fwd_x3", workspace, packed, split, out, acts, b, h, w, hu, wu, int(sin_mode))
    return out, acts


class DecodeMode3Function(torch.autograd.Function):
    """out = decoder(feat) on the HIP kernels, differentiable in feat and the 18 parameter tensors."""

    @staticmethod
    def forward(ctx, feat: torch.Tensor, hu: int, wu: int, sin_mode: int, *params: torch.Tensor) -> torch.Tensor:
        feat_c = checked_features(feat, params, PARAM_NAMES, PARAM_SHAPES, hu, wu, 2 * HIDDEN, " for decoder mode 3")
        packed = pack_on_device(params)
        out, acts = train_forward_mode3(feat_c, packed, hu, wu, sin_mode)
        ctx.save_for_backward(feat_c, acts, packed, *[p_.detach() for p_ in params])
        ctx.size = (hu, wu)
        return out

    @staticmethod
    def backward(ctx, gout: torch.Tensor):
        feat, acts, packed, *params = ctx.saved_tensors
        d_feat, d_params = backward_fused(gout.contiguous(), feat, acts, params, packed, ctx.size,
                                          need_feat_grad=ctx.needs_input_grad[0])
        return function_grads(ctx, d_feat, d_params, 4)


def train_forward_modes12(feat_c: torch.Tensor, params: Sequence[torch.Tensor], hu: int, wu: int, sin_mode: int, mode: int):
    """The modes-1/2 training forward on a contiguous fp32 CUDA ``feat_c``: the hoisted conv (diinn_precompute_P_wpu), the per-cell
    chain (diinn_cell_chain), decode_kernel<SIN, KPART=false, SAVE> (diinn_decode_train_fwd_qonly).
    Returns (out, acts [4,T,512,32], chain workspace [B,H,W,1024], packed image)."""
    b, _, h, w = feat_c.shape
    packed = pack_on_device(params, mode)
    acts, out, chain = train_buffers(feat_c, hu, wu)
    with _native.launcher(feat_c.device) as run:
        run("diinn_precompute_P_wpu", feat_c, packed, chain, b, h, w, 0, h)
        run("diinn_cell_chain", chain, packed, b, h, w, 0, h)
        run("diinn_decode_train_fwd_qonly", chain, packed, out, acts, b, h, w, hu, wu, int(sin_mode))
    return out, acts, chain, packed


class DecodeModes12Function(torch.autograd.Function):
    """out = decoder(feat) for decoder modes 1 and 2 on the HIP kernels, differentiable in feat and the 18 parameter tensors.
    Besides the planes the forward keeps the chain workspace (B*H*W*1024 floats): the masks and k_{i-1} of the chain's backward."""

    @staticmethod
    def forward(ctx, feat: torch.Tensor, hu: int, wu: int, sin_mode: int, mode: int, *params: torch.Tensor) -> torch.Tensor:
        feat_c = checked_features(feat, params, PARAM_NAMES, param_shapes(mode), hu, wu, 2 * HIDDEN, f" for decoder mode {mode}")
        out, acts, chain, packed = train_forward_modes12(feat_c, params, hu, wu, sin_mode, mode)
        ctx.save_for_backward(feat_c, acts, chain, packed, *[p_.detach() for p_ in params])
        ctx.size = (hu, wu)
        ctx.mode = mode
        return out

    @staticmethod
    def backward(ctx, gout: torch.Tensor):
        feat, acts, chain, packed, *params = ctx.saved_tensors
        d_feat, d_params = backward_fused_modes12(gout.contiguous(), feat, acts, chain, params, packed, ctx.size, ctx.mode,
                                                  need_feat_grad=ctx.needs_input_grad[0])
        return function_grads(ctx, d_feat, d_params, 5)


def decode_with_grad(decoder, feat: torch.Tensor, size: Sequence[int]) -> torch.Tensor:
    """``ImplicitDecoder.forward(x, size, None)`` under autograd (modes 1, 2 and 3; mode 4: mode4_training.decode_with_grad)."""
    params = named_params(decoder, PARAM_NAMES)
    hu, wu = size
    if decoder.mode in (1, 2):
        return DecodeModes12Function.apply(feat, int(hu), int(wu), int(decoder.sin_mode), int(decoder.mode), *params)
    return DecodeMode3Function.apply(feat, int(hu), int(wu), int(decoder.sin_mode), *params)
