"""The callers' side of the boundary: the reference's module
surface around the decoder, so its workflows run on the MI355X path unchanged.

  RDN / make_rdn     encoder, plain PyTorch-ROCm (north_star: "the encoder stays PyTorch-ROCm");
                     parameter names follow reference src/models/components/rdn.py:37-105 so
                     checkpoints load
  DIINN              reference diinn.py:8-19: encoder -> ImplicitDecoder (HIP kernels)
  make_net           reference sr_module.py:42-50
  SRLitModule        reference sr_module.py:62-194, the parts the inference callers use:
                     ctor hparams, ``net``, ``sub``/``div`` buffers, forward, step,
                     training_step / validation_step / test_step, configure_optimizers,
                     load_from_checkpoint.  pytorch_lightning is not required (it is absent from
                     the target image); scripts/train.py is the plain loop around these hooks.
"""
from __future__ import annotations

from types import SimpleNamespace
from typing import Any, Dict, Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import convs
from .convs import (_WINO4_G, _winograd_weight, pack_conv_ksplit, pack_conv_wino, pack_conv_wino4,  # noqa: F401  (re-exported:
                    pack_conv_x3)                                                                   # the weight images live in convs.py)
from .decoder import ImplicitDecoder
from .metrics import calc_psnr, psnr, resize_fn, ssim  # noqa: F401  (re-exported like the reference's sr_module)


# ---------------------------------------------------------------------------
# RDN encoder (config 'B': 16 blocks x 8 convs, growth 64), features only
# ---------------------------------------------------------------------------
class RDB_Conv(nn.Module):
    """3x3 conv + ReLU whose output is concatenated to its input (dense connection)."""

    def __init__(self, inChannels: int, growRate: int, kSize: int = 3):
        super().__init__()
        self.conv = nn.Sequential(nn.Conv2d(inChannels, growRate, kSize, padding=(kSize - 1) // 2), nn.ReLU())

    def forward(self, x):
        return torch.cat((x, self.conv(x)), 1)


class RDB(nn.Module):
    """Residual dense block: C dense convs, 1x1 local feature fusion, residual add."""

    def __init__(self, growRate0: int, growRate: int, nConvLayers: int, kSize: int = 3):
        super().__init__()
        self.convs = nn.Sequential(*[RDB_Conv(growRate0 + c * growRate, growRate, kSize) for c in range(nConvLayers)])
        self.LFF = nn.Conv2d(growRate0 + nConvLayers * growRate, growRate0, 1)

    def forward(self, x, hip_autograd: bool = False, max_pixels: Optional[int] = None):
        if not torch.is_grad_enabled():
            return self._forward_dense_buffer(x)
        if hip_autograd and self._hip_autograd_applies(x, max_pixels):
            from .encoder_training import RDBFunction, block_params
            return RDBFunction.apply(x, *block_params(self))
        return self.LFF(self.convs(x)) + x

    def _hip_autograd_applies(self, x, max_pixels) -> bool:
        """``RDN.hip_autograd``'s conditions for this block and input: CUDA fp32, the config-'B' block shape, and a map within
        the encoder's ``hip_trunk_max_pixels``; anything else trains through the framework as before."""
        from .encoder_training import block_applies
        return (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and max_pixels is not None
                and x.shape[0] * x.shape[-2] * x.shape[-1] <= max_pixels and self.LFF.weight.dtype == torch.float32
                and block_applies(self))

    def _forward_dense_buffer(self, x):
        """Inference form of the dense block: one [B, G0 + C*G, H, W] buffer, every conv reads the
        channels written so far and appends its G outputs in place -- the reference's
        ``torch.cat((x, out), 1)`` (rdn.py:15-17) re-copies the whole growing stack at every conv
        (2,816 channel-planes per block instead of 576).  Same arithmetic, same results."""
        b, g0, h, w = x.shape
        convs = list(self.convs)
        g = convs[0].conv[0].out_channels
        buf = x.new_empty((b, g0 + len(convs) * g, h, w))
        buf[:, :g0] = x
        c_in = g0
        for layer in convs:
            conv = layer.conv[0]
            buf[:, c_in:c_in + g] = F.relu(F.conv2d(buf[:, :c_in], conv.weight, conv.bias, padding=conv.padding))
            c_in += g
        return self.LFF(buf) + x


class RDN(nn.Module):
    _CONFIGS = {"A": (20, 6, 32), "B": (16, 8, 64)}
    # Inference (no autograd, fp32, config 'B') runs the whole encoder on the library's kernels:
    # SFENet1 on diinn_sfe1_forward, the 147 convolutions after it through diinn_rdn_forward_ex -- the split-K
    # kernel on small maps, Winograd 3x3 + streaming 1x1 kernels from 8192 pixels on.  Measured (tools/enc_trunk_time.py,
    # HIP vs MIOpen eager): 1.95 vs 7.6 ms at 48x48, 3.6 vs 7.6 at 96x96, 3.9 vs 8.1 at 128x128, 9.3 vs 20.2 at 192x192,
    # 11.8 vs 28.6 at 256x256, 28.3 vs 61.6 at 384x384, 47.0 vs 109.5 at 512x512.  The attribute caps the batch*H*W
    # that takes this path (workspace: 2,240 floats per pixel + 34.6 MB for the F(4x4) kernel's split); None disables it (MIOpen everywhere).
    hip_trunk_max_pixels: Optional[int] = 1024 * 1024          # byte offsets of a wave's channel slice stay far below 2^31
    # 3x3 layers as Winograd F(2x2, 3x3) (csrc/diinn_winograd.hip) on maps of >= 8192 pixels: 2.25x fewer MFMAs, fp32,
    # equal to the direct sum up to reassociation (~1e-6 relative).  False keeps every layer on the direct kernel.
    hip_winograd: bool = True
    # ... and as Winograd F(4x4, 3x3) (csrc/diinn_winograd4.hip) where that kernel needs fewer rounds of workgroups (from
    # about 190 x 190 pixels on: diinn_rdn_wino4_applies): 1.78x fewer MFMAs again; 256x256 11.8 -> 8.7 ms, 512x512 46.0 ->
    # 34.1 ms.  Per layer ~1e-5 of max|out| on unit-variance inputs (F(2x2): 4e-7); through the whole trunk 2e-6 absolute
    # at max|feat| 1.6 against MIOpen (F(2x2): 6e-7; the parity bound is 2e-5 x max).  False keeps F(2x2, 3x3) everywhere.
    hip_winograd4: bool = True
    # optional: the 3x3 layers in split-bf16 arithmetic on the bf16 MFMA (csrc/diinn_conv_x3.hip) on maps of >= 32,768
    # pixels: hi + lo bf16 operands, three products per term, fp32 accumulation; inside a dense block the activations are
    # exchanged already split.  Per layer ~4e-6 of max|out| against float64; the whole trunk differs from the fp32 one by
    # ~3e-6 of max|feat| and the decoded image by ~3e-8.  Measured per trunk: 192x192 9.4 -> 6.7 ms,
    # 256x256 11.85 -> 7.9 ms, 384x384 28.1 -> 20.1 ms, 512x512 46.6 -> 31.4 ms; below ~180x180 the Winograd kernels stay faster and are used.
    hip_split_bf16: bool = False
    # opt-in: under autograd the 16 residual dense blocks run on the library's kernels (encoder_training.RDBFunction, DESIGN.md
    # section 3.8: forward and input gradients on the trunk's convolution kernels, weight gradients on conv_wgrad_kernel), fp32 CUDA
    # maps of up to hip_trunk_max_pixels; SFENet1, SFENet2 and GFF stay on the framework.  False: autograd through the framework.
    hip_autograd: bool = False

    def __init__(self, G0: int = 64, RDNkSize: int = 3, RDNconfig: str = "B", n_colors: int = 3):
        super().__init__()
        self.D, C, G = self._CONFIGS[RDNconfig]
        pad = (RDNkSize - 1) // 2
        self.SFENet1 = nn.Conv2d(n_colors, G0, RDNkSize, padding=pad)
        self.SFENet2 = nn.Conv2d(G0, G0, RDNkSize, padding=pad)
        self.RDBs = nn.ModuleList([RDB(G0, G, C) for _ in range(self.D)])
        self.GFF = nn.Sequential(nn.Conv2d(self.D * G0, G0, 1), nn.Conv2d(G0, G0, RDNkSize, padding=pad))
        self.out_dim = G0
        self.args = SimpleNamespace(G0=G0, RDNkSize=RDNkSize, RDNconfig=RDNconfig, scale=[2],
                                    no_upsampling=True, n_colors=n_colors)
        self._hip_ok = (RDNconfig == "B" and G0 == 64 and RDNkSize == 3)
        self._hip_pack = None
        self._hip_key = None

    def _trunk_layers(self):
        """The 147 convolutions after SFENet1 in execution order (rdn.py:97-103)."""
        layers = [self.SFENet2]
        for rdb in self.RDBs:
            layers += [c.conv[0] for c in rdb.convs] + [rdb.LFF]
        return layers + [self.GFF[0], self.GFF[1]]

    def _hip_packed(self, device):
        layers = self._trunk_layers()
        key = (str(device),) + tuple((l.weight.data_ptr(), l.weight._version, l.bias._version) for l in layers)
        if self._hip_pack is None or self._hip_key != key:
            w = torch.cat([pack_conv_ksplit(l.weight) for l in layers]).to(device)
            b = torch.cat([l.bias.detach().to(torch.float32) for l in layers]).to(device)
            self._hip_pack, self._hip_key, self._hip_x3, self._hip_wu4, self._hip_wu2 = (w, b), key, None, None, None
        return self._hip_pack

    def _hip_packed_wino(self, device):
        """The F(2x2, 3x3) image of the 130 3x3 weights (152 MB), built on first use: a model that only sees maps whose
        3x3 layers run F(4x4, 3x3) (341 MB) or the split-K kernel (the 85 MB permutation above) never builds it.
        ``RDN.free_unused_images()`` drops the images again."""
        self._hip_packed(device)
        if getattr(self, "_hip_wu2", None) is None:
            self._hip_wu2 = torch.cat([pack_conv_wino(l.weight.to(device)) for l in self._trunk_layers()
                                       if l.kernel_size == (3, 3)]).to(device)
        return self._hip_wu2

    def free_unused_images(self, keep=()):
        """Drop the derived weight images (``"wino"`` F(2x2): 152 MB, ``"wino4"`` F(4x4): 341 MB, ``"x3"`` split bf16: 88 MB)
        that are not named in ``keep``; they are rebuilt on the next forward that needs them.  Images captured by a hipGraph
        entry stay alive with it."""
        for name, attr in (("wino", "_hip_wu2"), ("wino4", "_hip_wu4"), ("x3", "_hip_x3")):
            if name not in keep:
                setattr(self, attr, None)

    def _hip_packed_wino4(self, device):
        """The F(4x4, 3x3) image of the 130 3x3 weights, built on first use (and again when a weight changes)."""
        self._hip_packed(device)
        if getattr(self, "_hip_wu4", None) is None:
            self._hip_wu4 = torch.cat([pack_conv_wino4(l.weight.to(device)) for l in self._trunk_layers()
                                       if l.kernel_size == (3, 3)]).to(device)
        return self._hip_wu4

    def _hip_packed_x3(self, device):
        """The split-bf16 image of the 130 3x3 weights, built on first use (and again when a weight changes)."""
        self._hip_packed(device)
        if getattr(self, "_hip_x3", None) is None:
            layers = self._trunk_layers()
            # the 130 3x3 layers in execution order, then the 16 local-fusion 1x1 layers
            self._hip_x3 = torch.cat([pack_conv_x3(l.weight.to(device)) for l in layers if l.kernel_size == (3, 3)] +
                                     [pack_conv_x3(rdb.LFF.weight.to(device)) for rdb in self.RDBs]).to(device)
        return self._hip_x3

    # the F(4x4) kernel's split area and its sticky status word: ONE area per (device, stream) for every user in the process (convs.py)
    _w4_area = staticmethod(convs.w4_area)
    handoff_status = staticmethod(convs.handoff_status)

    def _forward_hip_trunk(self, shallow):
        import ctypes as C
        from . import _native
        lib = _native.load()
        b, _, h, w = shallow.shape
        shallow = shallow.contiguous()
        dev = shallow.device
        packed, biases = self._hip_packed(dev)
        x3 = self.hip_winograd and self.hip_split_bf16
        form = convs.conv_form(b, h, w)
        w4 = self.hip_winograd and self.hip_winograd4 and not x3 and form == "wino4"
        # the F(2x2) image only where a kernel reads it (~0.6 GB of weight copies for an 88 MB encoder otherwise)
        needs_wino = self.hip_winograd and not w4 and (x3 or form != "ksplit")
        algo = (_native.RDN_ALGO_X3 if x3 else _native.RDN_ALGO_WINO4 if w4 else _native.RDN_ALGO_WINO if needs_wino
                else _native.RDN_ALGO_DIRECT)
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731
        packed_wino = self._hip_packed_wino(dev) if needs_wino else None
        packed_w4 = self._hip_packed_wino4(dev) if w4 else None
        packed_x3 = self._hip_packed_x3(dev) if x3 else None
        planes = torch.empty(lib.diinn_rdn_planes_floats(algo, b, h, w), dtype=torch.float32, device=dev)
        area = self._w4_area(dev) if w4 else None
        out = torch.empty_like(shallow)
        with torch.cuda.device(dev):
            stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            _native.check(lib.diinn_rdn_forward_ex(stream, algo, ptr(shallow), ptr(packed), ptr(packed_wino), ptr(packed_w4),
                                                   ptr(packed_x3), ptr(biases), ptr(planes), ptr(area), ptr(out), b, h, w),
                          "diinn_rdn_forward_ex")
        return out

    def _sfe1_hip(self, x):
        """SFENet1 on the library's own kernel (diinn_sfe1_forward): the whole inference encoder then runs without a
        library convolution."""
        import ctypes as C
        from . import _native
        lib = _native.load()
        x = x.contiguous()
        b, c, h, w = x.shape
        wt, bias = self.SFENet1.weight.detach().contiguous(), self.SFENet1.bias.detach().contiguous()
        out = torch.empty((b, 64, h, w), dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            _native.check(lib.diinn_sfe1_forward(stream, C.c_void_p(x.data_ptr()), c, C.c_void_p(wt.data_ptr()),
                                                 C.c_void_p(bias.data_ptr()), C.c_void_p(out.data_ptr()), b, h, w),
                          "diinn_sfe1_forward")
        return out

    def forward(self, x):
        if (self._hip_ok and self.hip_trunk_max_pixels is not None and x.is_cuda and not torch.is_grad_enabled()
                and x.dtype == torch.float32 and x.shape[0] * x.shape[-2] * x.shape[-1] <= self.hip_trunk_max_pixels):
            if x.shape[1] <= 4 and self.SFENet1.weight.dtype == torch.float32:
                return self._forward_hip_trunk(self._sfe1_hip(x))
            return self._forward_hip_trunk(self.SFENet1(x))
        shallow = self.SFENet1(x)
        x = self.SFENet2(shallow)
        blocks = []
        hip_autograd = self.hip_autograd and self._hip_ok and torch.is_grad_enabled()
        for rdb in self.RDBs:
            x = rdb(x, True, self.hip_trunk_max_pixels) if hip_autograd else rdb(x)
            blocks.append(x)
        return self.GFF(torch.cat(blocks, 1)) + shallow


def make_rdn(G0=64, RDNkSize=3, RDNconfig="B", scale=2, no_upsampling=True):
    if not no_upsampling:
        raise NotImplementedError("DIINN uses RDN as a feature encoder only (no_upsampling=True)")
    return RDN(G0=G0, RDNkSize=RDNkSize, RDNconfig=RDNconfig)


# ---------------------------------------------------------------------------
# model assemblies
# ---------------------------------------------------------------------------
class _GraphReplay:
    """hipGraph replay of a whole inference forward (encoder convolutions + decoder kernels), one graph per
    (input shape, output size, parameter versions).  Small inputs are launch-bound in the encoder (48x48:
    ~7 ms eager for ~150 launches); the graph removes that.  The decoder's C-ABI launches never allocate
    or synchronise, so they capture as they are."""

    MAX_GRAPHS = 8

    def _init_graphs(self, graphs: bool):
        self.graphs = graphs
        self._graph_cache: Dict[Any, Any] = {}

    def _use_graph(self, x) -> bool:
        return self.graphs and x.is_cuda and not torch.is_grad_enabled()

    def _graph_key(self, x, size):
        """Everything that decides which kernels a capture records and which buffers they read: input geometry,
        output size, the identity and version of every parameter (a re-assigned ``param.data`` changes the
        pointer, an in-place update the version), and the knobs that switch code paths."""
        dec = getattr(self, "decoder", None)
        enc = getattr(self, "encoder", None)
        return (tuple(x.shape), x.dtype, x.device, int(size[0]), int(size[1]),
                tuple((p.data_ptr(), p._version) for p in self.parameters()),
                getattr(dec, "sin_mode", None), getattr(dec, "compute", None), getattr(dec, "mode", None),
                getattr(enc, "hip_trunk_max_pixels", None), getattr(enc, "hip_winograd", None),
                getattr(enc, "hip_split_bf16", None), getattr(enc, "hip_winograd4", None),
                getattr(dec, "hip_modes_split_bf16", None), getattr(self, "hip_hoisted", None),
                getattr(self, "hip_split_bf16", None))

    def _forward_graphed(self, x, size, bsize):
        key = self._graph_key(x, size)
        entry = self._graph_cache.get(key)
        if entry is None:
            if len(self._graph_cache) >= self.MAX_GRAPHS:
                self._graph_cache.pop(next(iter(self._graph_cache)))
            static_x = x.clone()
            side = torch.cuda.Stream(device=x.device)
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):                      # warm-up outside capture (MIOpen find, weight packing)
                for _ in range(2):
                    self._forward_eager(static_x, size, bsize)
            torch.cuda.current_stream().wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                # every buffer the captured kernels touch is either allocated inside the capture (the graph's
                # private pool: workspaces, activations, the result) or kept alive by the entry below (packed
                # weight images, which live in module caches that a later call may replace)
                static_y = self._forward_eager(static_x, size, bsize)
            keep = [getattr(m, a, None) for m in self.modules() for a in ("_packed", "_packed_split", "_packed_head", "_hip_pack", "_hip_x3", "_hip_wu4", "_hip_wu2", "_hoisted_images")]
            entry = (graph, static_x, static_y, keep)
            self._graph_cache[key] = entry
        graph, static_x, static_y = entry[:3]
        static_x.copy_(x)
        graph.replay()
        return static_y.clone()


class DIINN(nn.Module, _GraphReplay):
    """Reference diinn.py:8-19: ``decoder(encoder(x), size, bsize)``.  ``graphs=True`` (inference only)
    replays the whole forward from a hipGraph (see ``_GraphReplay``)."""

    def __init__(self, mode, init_q, graphs: bool = False):
        super().__init__()
        self.encoder = make_rdn()
        if graphs and init_q:
            raise NotImplementedError("DIINN(init_q=True, graphs=True): graph replay of the init_q decoder's chunk loop is not "
                                      "covered; construct with graphs=False")
        self.decoder = ImplicitDecoder(mode=mode, init_q=init_q)
        self._init_graphs(graphs)

    def _forward_eager(self, x, size, bsize=None):
        return self.decoder(self.encoder(x), size, bsize)

    def set_split_bf16(self, enabled: bool = True) -> "DIINN":
        """Switch both optional split-bf16 modes (not in the reference; DESIGN.md sections 3.5 and 3.9): the decoder's
        per-pixel layers (``decoder.compute = "bf16x3"``) and the encoder's 3x3 layers (``encoder.hip_split_bf16``).  The
        output stays within the reference tolerance (1e-4 x max(1, |ref|)); 256x256 x4: 17.9 -> 10.1 ms per forward."""
        self.decoder.compute = "bf16x3" if enabled else "f32"
        self.encoder.hip_split_bf16 = bool(enabled)
        return self

    def forward(self, x, size, bsize=None):
        if self._use_graph(x):
            return self._forward_graphed(x, size, bsize)
        return self._forward_eager(x, size, bsize)

    @torch.no_grad()
    def forward_sharded(self, x, size, src: int = 0, gather_to: Optional[int] = 0, group=None, mode: str = "halo"):
        """The same forward with the HR grid cut into row bands, one per rank of the process group (one process per
        GPU under ``torch.distributed``): rank ``src`` runs the encoder, every rank receives the
        LR feature rows its band reads (+ a one-row halo) and decodes its band, and the image is assembled on
        ``gather_to`` (returned there, ``None`` elsewhere) -- or, with ``gather_to=None``, every rank gets
        ``(band, (y0, y1))``.  Every rank passes ``x`` (only its shape is used away from ``src``).  Inference, mode 3.
        With one rank this is ``forward``.  The reference has no multi-GPU inference (benchmarks.py:13: devices=1)."""
        import torch.distributed as dist
        from . import sharded as S
        if self.decoder.mode == 4:
            raise NotImplementedError("forward_sharded does not cover mode 4 (its 3x3 head reads the neighbouring band's "
                                      "rows); use forward, which decodes mode 4 in row chunks on one GPU")
        if self.decoder.init_q and self.decoder.mode != 3 and self.decoder.hip_initq_modes:
            raise NotImplementedError("forward_sharded does not cover init_q=True with modes 1 and 2 (hip_initq_modes: the per-pixel "
                                      "chain has no band-sized form); use forward, which decodes in row chunks on one GPU")
        if self.decoder.mode in (1, 2) and self.decoder.compute == "bf16x3" and self.decoder.hip_modes_split_bf16:
            raise NotImplementedError("forward_sharded does not cover the split-bf16 arithmetic of modes 1 and 2 "
                                      "(hip_modes_split_bf16: no window or tile form); use forward")
        if not dist.is_initialized() or dist.get_world_size(group) == 1:
            out = self._forward_eager(x, size, None)
            return out if gather_to is not None else (out, (0, int(size[0])))
        if self.decoder.mode != 3 or self.decoder.init_q:
            raise NotImplementedError("forward_sharded covers the mode-3 decoder")
        hu, wu = size
        b, _, h, w = x.shape
        shape = (int(b), 64, int(h), int(w))
        packed = self.decoder.packed_weights(x.device)
        # the arithmetic and the sine mode are baked into a BandDecoder at construction: they are part of the key, so
        # switching ``decoder.compute`` / ``sin_mode`` (or ``set_split_bf16``) between two calls rebuilds it
        key = (shape, int(hu), int(wu), packed.data_ptr(), src, mode, id(group),
               self.decoder.compute, self.decoder.sin_mode)
        if getattr(self, "_band_key", None) != key:           # band-sized buffers are allocated once per geometry
            self._band_dec = S.BandDecoder(shape, (int(hu), int(wu)), packed, group=group, src=src, mode=mode,
                                           sin_mode=self.decoder.sin_mode, compute=self.decoder.compute)
            self._band_key = key
        dec = self._band_dec
        feat = self.encoder(x).contiguous() if dist.get_rank(group) == src else None
        band = dec.step(feat)
        if gather_to is None:
            return band, (dec.band.y0, dec.band.y1)
        return dec.gather(band, dst=gather_to)


class MLP(nn.Module):
    """Linear/ReLU stack with the reference's parameter names ``layers.{0,2,4,...}`` (mlp.py:3-20)."""

    def __init__(self, in_dim, out_dim, hidden_list):
        super().__init__()
        layers, last = [], in_dim
        for width in hidden_list:
            layers += [nn.Linear(last, width), nn.ReLU()]
            last = width
        layers.append(nn.Linear(last, out_dim))
        self.layers = nn.Sequential(*layers)

    def forward(self, x):
        return self.layers(x.reshape(-1, x.shape[-1])).view(*x.shape[:-1], -1)


class LIIF(nn.Module, _GraphReplay):
    """The LIIF comparison model (reference liif.py:9-155; Chen et al. 2021) behind the same
    ``forward(inp, size, bsize=None)`` boundary: RDN encoder (PyTorch-ROCm) + the implicit MLP decoder on
    the HIP path (``liif_kernel``).  Constructor defaults only (local ensemble, feature unfolding, cell
    decoding -- what ``make_net('liif')`` builds, sr_module.py:45-46).

    ``hip_autograd`` (a plain attribute, also a constructor keyword; default False): with it set, a call under autograd with
    ``bsize=None`` -- the reference's training call, sr_module.py:127-129 -- runs the decoder through
    ``liif_training.LIIFFunction`` (the inference kernels saving the activations, the backward pass on the HIP kernels; ROCm GPU
    only), and with ``bsize`` given the decode runs under no_grad like the reference's ``batched_predict`` (liif.py:129-140): the
    output carries no graph.  With it unset a call under autograd raises NotImplementedError, as it always did.  ``bsize`` itself
    is the reference's query-chunk size, a memory knob: accepted and ignored.  Graph replay is inference-only.

    ``hip_split_bf16`` (a plain attribute, also a constructor keyword; default False; not in the reference; named after the
    encoder's switch): the three hidden 256 x 256 layers of the decoder in split-bf16 arithmetic (``liif_x3_kernel`` through
    ``liif_decode_features(..., split=...)``) -- within the reference tolerance, 1e-4 x max(1, max|ref|),
    but not ``liif_kernel``'s bits, which the fixtures pin: hence a switch.  On its own it is inference only: the training forward
    (``hip_autograd`` under autograd with ``bsize=None``) refuses while it is set, unless ``hip_autograd_split_bf16`` is set too; the
    no_grad decode of a call with ``bsize`` honours it.  ``set_split_bf16`` sets it together with the encoder's.

    ``hip_autograd_split_bf16`` (a plain attribute, also a constructor keyword; default False; not in the state dict; not in the
    reference; named after ``ImplicitDecoder``'s switch): acts only together with ``hip_autograd`` AND ``hip_split_bf16``.  With all
    three set, a call under autograd with ``bsize=None`` trains with the three hidden layers in split-bf16 arithmetic both ways:
    ``liif_split_training.LIIFSplitFunction`` -- the forward is ``liif_x3_kernel``'s arithmetic saving the activations (the output
    under grad is the no_grad split output bit for bit), the backward chain runs on ``liif_bwd_layer_x3_kernel``, everything behind
    it stays fp32.  With ``hip_split_bf16`` unset it changes nothing: fp32 training.  ``set_split_bf16`` does
    not touch it."""

    hip_autograd = False
    hip_split_bf16 = False
    hip_autograd_split_bf16 = False

    def __init__(self, local_ensemble=True, feat_unfold=True, cell_decode=True, graphs: bool = False, hip_autograd: bool = False,
                 hip_split_bf16: bool = False, hip_autograd_split_bf16: bool = False):
        super().__init__()
        self._init_graphs(graphs)
        if not (local_ensemble and feat_unfold and cell_decode):
            raise NotImplementedError("the HIP path implements LIIF with local_ensemble, feat_unfold and cell_decode on")
        self.local_ensemble, self.feat_unfold, self.cell_decode = local_ensemble, feat_unfold, cell_decode
        self.hip_autograd = bool(hip_autograd)
        self.hip_split_bf16 = bool(hip_split_bf16)
        self.hip_autograd_split_bf16 = bool(hip_autograd_split_bf16)
        self.encoder = make_rdn()
        self.imnet = MLP(self.encoder.out_dim * 9 + 4, 3, [256, 256, 256, 256])
        self._packed = None
        self._packed_split = None                                # the split training image of _packed: built on first use, same key
        self._packed_key = None

    def gen_feat(self, inp):
        return self.encoder(inp)

    def _packed_weights(self, device):
        from .decoder import pack_liif_state_dict
        key = (str(device),) + tuple((p.data_ptr(), p._version) for p in self.imnet.parameters())
        if self._packed is None or self._packed_key != key:
            self._packed = pack_liif_state_dict(self.imnet.state_dict(), prefix="").to(device)
            self._packed_split = None
            self._packed_key = key
        return self._packed

    def _split_weights(self, device):
        """The split training image of ``_packed_weights(device)``, cached beside it under its key (the module holds on to it: a
        graph entry keeps it alive)."""
        from .decoder import pack_liif_split
        packed = self._packed_weights(device)
        if self._packed_split is None:
            self._packed_split = pack_liif_split(packed).to(device)
        return packed, self._packed_split

    def set_split_bf16(self, enabled: bool = True) -> "LIIF":
        """Switch both optional split-bf16 modes (not in the reference): the decoder's hidden layers (``hip_split_bf16``) and the
        encoder's 3x3 layers (``encoder.hip_split_bf16``), as ``DIINN.set_split_bf16`` does."""
        self.hip_split_bf16 = bool(enabled)
        self.encoder.hip_split_bf16 = bool(enabled)
        return self

    def _forward_eager(self, inp, size, bsize=None):
        from .decoder import liif_decode_features
        feat = self.gen_feat(inp)
        if self.hip_split_bf16:
            packed, split = self._split_weights(feat.device)
            return liif_decode_features(feat, packed, size, split=split)
        return liif_decode_features(feat, self._packed_weights(feat.device), size)

    def _forward_train(self, inp, size, split: bool = False):
        if split:
            from .liif_split_training import decode_with_grad
        else:
            from .liif_training import decode_with_grad
        if not inp.is_cuda:
            raise RuntimeError("diinn_amd: the training forward runs on a ROCm GPU only (no CPU implementation)")
        return decode_with_grad(self.imnet, self.gen_feat(inp), size)

    def forward(self, inp, size, bsize=None):
        if torch.is_grad_enabled() and self.hip_autograd:
            if inp.requires_grad or any(p.requires_grad for p in self.parameters()):
                if bsize is None:
                    if self.hip_split_bf16 and self.hip_autograd_split_bf16:
                        return self._forward_train(inp, size, split=True)
                    if self.hip_split_bf16:
                        raise NotImplementedError("diinn_amd: LIIF trains in fp32 only: unset LIIF.hip_split_bf16 (the split-bf16 "
                                                  "decoder is inference-only), or call under torch.no_grad()")
                    return self._forward_train(inp, size)
                with torch.no_grad():                            # batched_predict is no_grad in the reference: no graph
                    return self._forward_eager(inp, size, bsize)
        elif torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            raise NotImplementedError("diinn_amd: LIIF under autograd is opt-in: set LIIF.hip_autograd = True (the decoder then trains "
                                      "on the HIP kernels), or call under torch.no_grad()")
        if self._use_graph(inp):
            return self._forward_graphed(inp, size, bsize)
        return self._forward_eager(inp, size, bsize)


class MetaSR(nn.Module, _GraphReplay):
    """The MetaSR comparison model (reference metasr.py:22-135; Hu et al. 2019 as re-implemented by LIIF)
    behind ``forward(inp, size, bsize=None)``: RDN encoder (PyTorch-ROCm) + the meta-upscale decoder on the
    HIP path (``metasr_kernel``).  Under autograd with ``bsize=None`` -- the reference's training call, sr_module.py:127-129 --
    the decoder runs through ``metasr_training.MetaSRFunction`` (the same forward kernels, the per-cell backward on the HIP
    kernels; ROCm GPU only).  With ``bsize`` given the reference decodes under no_grad (``batched_predict``, metasr.py:106-117):
    the output carries no graph, and ``bsize`` itself, a memory knob, is ignored.  Graph replay is inference-only.

    ``hip_hoisted`` (a plain attribute, also a constructor keyword; default False; not in the reference): the decoder in its hoisted
    form -- the 3x3 conv [M; B0] per LR cell (``diinn_precompute_P_wpu``), then ``metasr_hoisted_kernel`` turns M into pixels
    (``decoder.metasr_decode_hoisted``) -- in inference and, under autograd, as the forward of ``MetaSRHoistedFunction`` (the same two
    launches on the same device-gathered image: the output under grad is the no_grad output bit for bit; the backward is
    unchanged).  The output is within the reference tolerance but not metasr_kernel's bits, which the fixtures pin: hence a
    switch.  Measured (profiles/metasr_hoisted_times.txt): decode 17x and training step 4x faster at x4,
    2x / 1.5x at x1, 1.1x / 1.3x when down-scaling; no scale was found at which the direct kernel wins."""

    hip_hoisted = False

    def __init__(self, graphs: bool = False, hip_hoisted: bool = False):
        super().__init__()
        self._init_graphs(graphs)
        self.hip_hoisted = bool(hip_hoisted)
        self.encoder = make_rdn()
        self.imnet = MLP(3, self.encoder.out_dim * 9 * 3, [256])
        self._packed = None
        self._packed_key = None
        self._hoisted_images = None                              # (packed, image, wx) of the last hoisted decode: a graph entry keeps them

    def gen_feat(self, inp):
        self.feat = self.encoder(inp)
        return self.feat

    def _packed_weights(self, device):
        from .decoder import pack_metasr_state_dict
        key = (str(device),) + tuple((p.data_ptr(), p._version) for p in self.imnet.parameters())
        if self._packed is None or self._packed_key != key:
            self._packed = pack_metasr_state_dict(self.imnet.state_dict(), prefix="").to(device)
            self._packed_key = key
        return self._packed

    def _forward_eager(self, inp, size, bsize=None):
        from .decoder import metasr_decode_features, metasr_decode_hoisted
        feat = self.gen_feat(inp)
        if self.hip_hoisted:
            from .metasr_training import PARAM_NAMES, images_on_device
            from .training import named_params
            # (gathered on the device, cached per weight version in a cache that may evict them: the module holds on to them)
            self._hoisted_images = images_on_device(named_params(self.imnet, PARAM_NAMES))
            packed, image, _ = self._hoisted_images
            return metasr_decode_hoisted(feat, packed, image, size)
        return metasr_decode_features(feat, self._packed_weights(feat.device), size)

    def _forward_train(self, inp, size):
        from .metasr_training import decode_with_grad
        if not inp.is_cuda:
            raise RuntimeError("diinn_amd: the training forward runs on a ROCm GPU only (no CPU implementation)")
        return decode_with_grad(self.imnet, self.gen_feat(inp), size, hoisted=self.hip_hoisted)

    def forward(self, inp, size, bsize=None):
        if torch.is_grad_enabled() and (inp.requires_grad or any(p.requires_grad for p in self.parameters())):
            if bsize is None:
                return self._forward_train(inp, size)
            with torch.no_grad():                                # batched_predict is no_grad in the reference: no graph
                return self._forward_eager(inp, size, bsize)
        if self._use_graph(inp):
            return self._forward_graphed(inp, size, bsize)
        return self._forward_eager(inp, size, bsize)


class BICUBIC_NET(nn.Module):
    """Antialiased bicubic resize baseline (reference sr_module.py:53-60 via torchvision.Resize,
    which lowers to this interpolate call)."""

    def forward(self, x, size, eval_bsize=None):
        return F.interpolate(x, size=tuple(int(s) for s in size), mode="bicubic", align_corners=False, antialias=True)


def make_net(arch, mode, init_q):
    if arch == "diinn":
        return DIINN(mode=mode, init_q=init_q)
    if arch == "bicubic":
        return BICUBIC_NET()
    if arch == "liif":
        return LIIF()
    if arch == "metasr":
        return MetaSR()
    return None   # the reference's make_net falls through to None for unknown names


class SRLitModule(nn.Module):
    """Inference surface of the reference LightningModule (sr_module.py:62-125)."""

    def __init__(self, arch: str, mode: int = 1, init_q: bool = False, lr: float = 1e-4, lr_gamma: float = 0.5,
                 lr_step: int = 10, eval_bsize: int = 30000):
        super().__init__()
        self.hparams = SimpleNamespace(arch=arch, mode=mode, init_q=init_q, lr=lr, lr_gamma=lr_gamma,
                                       lr_step=lr_step, eval_bsize=eval_bsize)
        self.net = make_net(arch, mode, init_q)
        self.register_buffer("sub", torch.FloatTensor([0.5]).view(1, -1, 1, 1))
        self.register_buffer("div", torch.FloatTensor([0.5]).view(1, -1, 1, 1))
        self.criterion = nn.L1Loss()

    def forward(self, x: torch.Tensor, size, eval_bsize=None):
        return self.net(x, size, eval_bsize)

    def forward_sharded(self, x: torch.Tensor, size, **kw):
        """``forward`` with the HR grid sharded by row bands over the ranks of ``torch.distributed`` (DIINN only)."""
        if not hasattr(self.net, "forward_sharded"):
            raise NotImplementedError(f"arch {self.hparams.arch}: only DIINN has a sharded forward")
        return self.net.forward_sharded(x, size, **kw)

    def step(self, batch: Any, eval_bsize=None):
        """Boundary restatement, not new design: this loop IS reference sr_module.py:113-125 (``batch`` maps scale ->
        (lr, hr, name); normalise by sub/div, decode to the HR size, L1, de-normalise and clamp), kept statement for
        statement because ``training_step`` / ``validation_step`` / ``test_step`` and any user subclass depend on its exact
        return value ``(mean loss, {scale: prediction in [0, 1]})``."""
        loss = 0
        pred_hrs: Dict[Any, torch.Tensor] = {}
        for scale in batch:
            lr, hr, _ = batch[scale]
            lr = (lr - self.sub) / self.div
            hr = (hr - self.sub) / self.div
            pred_hr = self.forward(lr, hr.shape[-2:], eval_bsize)
            loss += self.criterion(pred_hr, hr)
            pred_hrs[scale] = (pred_hr * self.div + self.sub).clamp_(0, 1)
        return loss / len(batch), pred_hrs

    def training_step(self, batch: Any, batch_idx: int = 0):
        """sr_module.py:127-137: the decoder runs under autograd with bsize=None (training.py: HIP forward
        with saved planes + HIP backward)."""
        loss, _ = self.step(batch)
        return {"loss": loss}

    @torch.no_grad()
    def validation_step(self, batch: Any, batch_idx: int = 0):
        """sr_module.py:143-154: loss and the DIV2K-style PSNR (border shaved by the scale) per scale."""
        loss, pred_hrs = self.step(batch, self.hparams.eval_bsize)
        res = {"val/loss": loss}
        for scale in batch:
            res[f"val/psnr_x{scale}"] = calc_psnr(pred_hrs[scale], batch[scale][1], dataset="div2k", scale=scale, rgb_range=1)
        return res

    def configure_optimizers(self):
        """Boundary restatement of sr_module.py:185-194 (the return shape is Lightning's contract): Adam(lr) +
        StepLR(lr_step, lr_gamma), one scheduler step per epoch."""
        optimizer = torch.optim.Adam(self.parameters(), lr=self.hparams.lr)
        scheduler = torch.optim.lr_scheduler.StepLR(optimizer=optimizer, step_size=self.hparams.lr_step,
                                                    gamma=self.hparams.lr_gamma)
        return [optimizer], [scheduler]

    def checkpoint(self) -> Dict[str, Any]:
        """The two entries of a Lightning checkpoint that ``load_from_checkpoint`` (here and in the reference) reads."""
        return {"state_dict": self.state_dict(), "hyper_parameters": dict(vars(self.hparams))}

    @torch.no_grad()
    def test_step(self, batch: Any, batch_idx: int = 0, dataloader_idx: Optional[int] = None):
        """sr_module.py:159-180: decode with the checkpoint's eval_bsize, then PSNR, SSIM and the PSNR of
        the re-downsampled prediction against the re-downsampled target, per scale (data_range=1)."""
        _, pred_hrs = self.step(batch, self.hparams.eval_bsize)
        res = {}
        for scale in batch:
            hr = batch[scale][1]
            lr_size = (round(hr.shape[-2] / scale), round(hr.shape[-1] / scale))
            res[scale] = {
                "psnr_res": psnr(pred_hrs[scale], hr, data_range=1),
                "ssim_res": ssim(pred_hrs[scale], hr, data_range=1),
                "lr_psnr_res": psnr(resize_fn(pred_hrs[scale], lr_size), resize_fn(hr, lr_size), data_range=1),
            }
        return res

    @classmethod
    def load_from_checkpoint(cls, checkpoint_path: str, map_location=None, strict: bool = True, **overrides):
        """Lightning checkpoint dict: ``hyper_parameters`` (ctor kwargs saved by save_hyperparameters,
        sr_module.py:91) and ``state_dict`` (keys ``net.encoder.*``, ``net.decoder.*``, ``sub``, ``div``)."""
        # plain tensors + a dict of primitives load under weights_only=True; a checkpoint that pickles other
        # classes (Lightning's AttributeDict, callbacks, LightningCLI namespaces) executes code on load and needs an
        # explicit opt-in: DIINN_TRUST_CKPT=1 (README "Checkpoints")
        import os
        try:
            ckpt = torch.load(checkpoint_path, map_location=map_location or "cpu", weights_only=True)
        except Exception as e:
            if os.environ.get("DIINN_TRUST_CKPT") == "1":
                ckpt = torch.load(checkpoint_path, map_location=map_location or "cpu", weights_only=False)
            else:
                raise RuntimeError(
                    f"{checkpoint_path} did not load as plain tensors (torch.load(weights_only=True): "
                    f"{type(e).__name__}: {e}).  Checkpoints written by Lightning / LightningCLI can pickle their own "
                    f"classes; unpickling those runs code from the file.  If you trust this file, set "
                    f"DIINN_TRUST_CKPT=1 to load it with weights_only=False.") from e
        hp = dict(ckpt.get("hyper_parameters", {}))
        hp.update(overrides)
        known = ("arch", "mode", "init_q", "lr", "lr_gamma", "lr_step", "eval_bsize")
        model = cls(**{k: v for k, v in hp.items() if k in known})
        model.load_state_dict(ckpt["state_dict"], strict=strict)
        return model.eval()
