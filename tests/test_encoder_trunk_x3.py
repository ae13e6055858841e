"""The encoder trunk in split-bf16 arithmetic (RDN.hip_split_bf16; csrc/diinn_conv_x3.hip), block by block and layer by layer.

Inside a dense block the activations travel in the split format only ([b][group of 8 channels][hi, lo][H*W] x 16 bytes), through
kernels without an entry point of their own: conv3x3_x3_kernel<.., SPLIT_IN = true, ..>, conv3x3_x3m_kernel, conv1x1_x3_kernel
and the xs_out epilogue of all of them.  diinn_rdn_forward_ex works in a caller-owned ``planes`` buffer, and after a
DIINN_RDN_ALGO_X3 forward that buffer still holds every block's fp32 output (the global-fusion input), block 15's eight dense
outputs as split pairs (groups 8..71 of the split buffer) and block 15's output as a split pair (groups 0..7).  So every block
and every dense layer of the last block is compared, on the kernel's OWN input, with a float64 evaluation -- next to the
emulation sheet of the same arithmetic (convs.conv_x3_reference / rdb_x3_reference) on the same input and against the same
float64 values: the kernel may be at most R times as far from float64 as the sheet is.

The CPU tests show what that rule can see: each of four faults of a split-format kernel (a lost lo half on a vector, on an edge
pixel, in a whole layer; a dropped w_lo.x_hi product on a channel tail), applied to the sheet, moves the worst block at least
3.5x and the worst layer at least 10x away from float64; so R may not exceed 3.  A fifth (lo truncated instead of rounded) stays
below 2x and is caught by the bit-exact check of the stored pairs instead.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import diinn_amd.synth as synth
from diinn_amd import convs

# the cap of R: the weakest fault reaches 3.5x at block level (test_sheet_faults_are_seen)
R_CAP = 3.0
# dist_kernel <= R * dist_sheet.  Measured on the MI355X over every case below (5 maps x 2 weight sets x 5 kernel forms), worst
# dist_kernel / dist_sheet: per block 1.27, tail 1.13, per dense layer of block 15 1.67.  R = the worst x 1.5, rounded up to one
# decimal (1.672 x 1.5 = 2.51); the margin covers the order of the fp32 sums inside a product, which the sheet does not model
R = 2.6
assert R <= R_CAP

# the smallest maps that reach each edge: one pixel (all halo); a plane below 32; the batch stride of the split buffer, one column
# in the second 32-pixel tile and a ragged last row group; W = 1 and a second workgroup of conv1x1_x3_kernel that owns a single
# pixel; three column tiles and a plane that is no multiple of 64
MAPS = [(1, 1, 1), (1, 5, 3), (2, 9, 33), (1, 257, 1), (1, 13, 70)]
WSETS = ["default", "gained"]
GAIN, GAIN_SEED = 2.0, 77       # picked on the CPU: test_gained_weights_keep_every_dense_layer_alive
FILL = 0x7FC17FC1               # a NaN as float32 and as each of its two bf16 halves


@functools.lru_cache(maxsize=None)
def _encoder(wset):
    """The CPU encoder of a weight set: default init (seeded), or the synthetic weights with a gain of its own in every layer
    (at default init the residual dominates every block's output; with gains the dense layers carry weight)."""
    import diinn_amd.modules as M
    torch.manual_seed(3)
    enc = M.make_rdn()
    if wset == "gained":
        shapes = {k: list(v.shape) for k, v in enc.state_dict().items()}
        enc.load_state_dict({k: torch.from_numpy(v) for k, v in
                             synth.state_dict_for(shapes, 123, "enc.", gain=GAIN, layer_gain_seed=GAIN_SEED).items()})
    return enc.eval().requires_grad_(False)


def _image(b, h, w):
    return torch.from_numpy(synth.uniform(7, f"img:{b}x{h}x{w}", (b, 3, h, w), 0.5) + np.float32(0.5))


def _conv64(x64, conv, relu=False):
    y = F.conv2d(x64, conv.weight.double(), conv.bias.double(), padding=conv.padding)
    return y.relu() if relu else y


def _rdb64(block, x64):
    """One residual dense block in float64."""
    buf = x64
    for layer in block.convs:
        buf = torch.cat([buf, _conv64(buf, layer.conv[0], relu=True)], 1)
    return _conv64(buf, block.LFF) + x64


def _dist(a, ref64):
    return float((a.double() - ref64).abs().max() / ref64.abs().max())


def _bits(t):
    return t.contiguous().view(torch.int32)


def _layer_dists(block, x, dense_hi, dense_lo, sheet=False):
    """Per dense layer c of ``block``: the distance of its stored output (hi + lo) to float64 ReLU(conv) of its own inputs -- the
    fp32 block input ``x`` and the stored pairs of the layers before it -- relative to max|float64 output|; with ``sheet`` also the
    emulation sheet's distance on the same inputs."""
    x_hi, x_lo = convs.split_pair(x)
    got, ref = [], []
    for c, layer in enumerate(block.convs):
        conv = layer.conv[0]
        d_hi, d_lo = dense_hi[:, :64 * c], dense_lo[:, :64 * c]
        want = _conv64(torch.cat([x.double(), d_hi.double() + d_lo.double()], 1), conv, relu=True)
        sl = slice(64 * c, 64 * c + 64)
        got.append(_dist(dense_hi[:, sl].double() + dense_lo[:, sl].double(), want))
        if sheet:
            _, s_hi, s_lo = convs.conv_x3_reference(torch.cat([x_hi, d_hi], 1), torch.cat([x_lo, d_lo], 1), conv.weight, conv.bias, 1)
            ref.append(_dist(s_hi.double() + s_lo.double(), want))
    return got, ref


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the weight image, the sheets' own discrimination, the gained weight set


def _decode_x3_image(image, cin, k):
    """pack_conv_x3's image by the layout its docstring states, index by index: [group Cin/16][tap][M-tile 2][hi, lo][lane 64]
    [8 bf16], cout = 32 mt + (lane & 31), input channel = 16 group + 8 (lane >> 5) + j."""
    img = image.numpy().view(np.int16).reshape(cin // 16, k * k, 2, 2, 64, 8)
    co, ci, tap = np.meshgrid(np.arange(64), np.arange(cin), np.arange(k * k), indexing="ij")
    lane = (co & 31) + 32 * ((ci % 16) // 8)
    parts = [img[ci // 16, tap, co // 32, part, lane, ci % 8].reshape(64, cin, k, k) for part in (0, 1)]
    return [torch.from_numpy(np.ascontiguousarray(p)) for p in parts]


@pytest.mark.parametrize("cin,k", [(16, 3), (64, 3), (320, 3), (576, 3), (576, 1)])
def test_pack_conv_x3_layout(cin, k):
    """Every weight of the image is hi = bf16(w) and lo = bf16(w - hi), bit for bit, at the place the docstring states;
    unpack_conv_x3 is its inverse."""
    torch.manual_seed(100 * cin + k)
    w = (torch.rand(64, cin, k, k) * 2 - 1) / (cin * k * k) ** 0.5 * 1.7
    image = convs.pack_conv_x3(w)
    assert image.dtype == torch.float32 and image.numel() == k * k * 64 * cin
    hi = w.to(torch.bfloat16)
    lo = (w - hi.to(torch.float32)).to(torch.bfloat16)
    got_hi, got_lo = _decode_x3_image(image, cin, k)
    assert torch.equal(got_hi, hi.view(torch.int16)) and torch.equal(got_lo, lo.view(torch.int16))
    un_hi, un_lo = convs.unpack_conv_x3(image, cin, k)
    assert torch.equal(un_hi, hi.to(torch.float32)) and torch.equal(un_lo, lo.to(torch.float32))
    assert bool((un_lo != 0).any())


def test_trunk_x3_image_is_the_layers_in_order():
    """RDN._hip_packed_x3: diinn_rdn_x3_packed_floats() floats, the 130 3x3 images in _trunk_layers() order, then the 16 LFF images."""
    import diinn_amd._native as N
    enc = _encoder("gained")
    image = enc._hip_packed_x3("cpu")
    enc._hip_pack = enc._hip_key = enc._hip_x3 = None            # (the shared encoder keeps no 170 MB of images)
    assert image.numel() == N.load().diinn_rdn_x3_packed_floats()
    layers3 = [l for l in enc._trunk_layers() if l.kernel_size == (3, 3)]
    assert len(layers3) == 130
    offs = np.concatenate([[0], np.cumsum([l.weight.numel() for l in layers3])])
    for i in (0, 68, 129):                                       # SFENet2, the Cin = 256 dense layer of block 8, GFF.1
        assert torch.equal(_bits(image[offs[i]:offs[i + 1]]), _bits(convs.pack_conv_x3(layers3[i].weight))), i
    assert layers3[68].weight.shape[1] == 256
    base = int(offs[-1])
    for d in (0, 7, 15):
        sl = image[base + d * 64 * 576: base + (d + 1) * 64 * 576]
        assert torch.equal(_bits(sl), _bits(convs.pack_conv_x3(enc.RDBs[d].LFF.weight))), d
    assert base + 16 * 64 * 576 == image.numel()


def _chain(enc, x0, fault=None):
    """The 16 blocks through the sheets (``fault`` applied; 'lo_layer' to the last block only, as the table of faults has it).
    Returns per block its distance to float64 on its own fp32 input, per dense layer of the last block the same, and whether every
    stored block output is the canonical pair of its fp32 value."""
    x, blocks, canonical = x0, [], True
    for d, block in enumerate(enc.RDBs):
        f = None if (fault == "lo_layer" and d != 15) else fault
        out, out_hi, out_lo, dense_hi, dense_lo = convs.rdb_x3_reference(block, x, fault=f)
        blocks.append(_dist(out, _rdb64(block, x.double())))
        hi, lo = convs.split_pair(out)
        canonical = canonical and torch.equal(_bits(out_hi), _bits(hi)) and torch.equal(_bits(out_lo), _bits(lo))
        if d == 15:
            layers, _ = _layer_dists(block, x, dense_hi, dense_lo)
        x = out
    return blocks, layers, canonical


@functools.lru_cache(maxsize=None)
def _sound_chain(wset):
    enc = _encoder(wset)
    x0 = enc.SFENet2(enc.SFENet1(_image(1, 12, 13)))
    return x0, _chain(enc, x0)


@pytest.mark.parametrize("wset", WSETS)
@pytest.mark.parametrize("fault", convs.X3_FAULTS)
def test_sheet_faults_are_seen(wset, fault):
    """What the GPU tests below can see, shown on the sheets (12 x 13 map): with each of the first four faults the worst block is at
    least 3.5x, and the worst dense layer of the last block at least 10x, as far from float64 as on the sound sheet -- also block by
    block / layer by layer, which is how the GPU tests compare -- so a kernel with that fault fails dist_kernel <= R dist_sheet for
    every R <= 3.  Truncated lo halves stay below the cap: the worst block moves by at most 1.5x (measured 1.4x); a dense layer's
    distance IS the rounding of its stored pair (2^-17 of the value's binade, measured 8e-6 of max|out|), truncation's error is at
    most twice rounding's, so the worst layer moves by at most 2x (measured 1.7x default init, 1.9x gained -- not the 1.5x first
    expected of it).  Neither rule may be relied on to see it: it breaks the canonical-pair check of the stored output."""
    enc = _encoder(wset)
    x0, (blocks0, layers0, canonical0) = _sound_chain(wset)
    assert canonical0
    blocks, layers, canonical = _chain(enc, x0, fault)
    rb, rl = max(blocks) / max(blocks0), max(layers) / max(layers0)
    rb_each = max(a / b for a, b in zip(blocks, blocks0))
    rl_each = max(a / b for a, b in zip(layers, layers0))
    print(f"{wset} {fault}: sound worst block {max(blocks0):.2e} layer {max(layers0):.2e}; faulty {max(blocks):.2e} ({rb:.1f}x, "
          f"block by block {rb_each:.1f}x) layer {max(layers):.2e} ({rl:.1f}x, layer by layer {rl_each:.1f}x)")
    if fault == "trunc":
        assert 1 / 1.5 <= rb <= 1.5 and 1 / 1.5 <= rl <= 2.0
        assert not canonical
    else:
        assert rb >= 3.5 and rl >= 10
        assert rb_each >= 3.5 and rl_each >= 10
        assert R_CAP < 3.5


def test_gained_weights_keep_every_dense_layer_alive():
    """The gained weight set is kept only if, in float64, every dense layer of every block has an output RMS within [1/4, 4] of its
    block input's RMS (no layer dead, none blown up), so that every layer's arithmetic weighs in its block's output."""
    enc = _encoder("gained")
    x = _conv64(_conv64(_image(1, 12, 13).double(), enc.SFENet1), enc.SFENet2)
    rms = lambda t: float(t.pow(2).mean().sqrt())                # noqa: E731
    for d, block in enumerate(enc.RDBs):
        buf = x
        for c, layer in enumerate(block.convs):
            y = _conv64(buf, layer.conv[0], relu=True)
            assert 0.25 <= rms(y) / rms(x) <= 4.0, (d, c, rms(y) / rms(x))
            buf = torch.cat([buf, y], 1)
        x = _conv64(buf, block.LFF) + x


# ---------------------------------------------------------------------------------------------------------------------
# GPU: one forward per (map, weight set, kernel form), read back whole


@functools.lru_cache(maxsize=None)
def _device_encoder(wset):
    import copy
    return copy.deepcopy(_encoder(wset)).to(torch.device("cuda:0"))


@functools.lru_cache(maxsize=None)
def _forward_x3(wset, shape, rows):
    """diinn_rdn_forward_ex(DIINN_RDN_ALGO_X3) with DIINN_ENC_X3_MIN = 0 and DIINN_ENC_X3_ROWS = ``rows`` (the caller's ``knobs``
    fixture restores both) in a ``planes`` buffer of its own, prefilled with NaN patterns and followed by a guard of 4096 floats in
    the same allocation.  Returns CPU tensors: sfe1, out, and planes + guard as int32."""
    import diinn_amd._native as N
    lib = N.load()
    dev = torch.device("cuda:0")
    b, h, w = shape
    enc = _device_encoder(wset)
    N.debug_set("DIINN_ENC_X3_MIN", 0)
    N.debug_set("DIINN_ENC_X3_ROWS", rows)
    with torch.no_grad():
        sfe1 = enc._sfe1_hip(_image(b, h, w).to(dev))
    packed, biases = enc._hip_packed(dev)
    wino, x3 = enc._hip_packed_wino(dev), enc._hip_packed_x3(dev)
    n = lib.diinn_rdn_planes_floats(N.RDN_ALGO_X3, b, h, w)
    assert n == b * h * w * (2 * 576 + 1024 + 64 + 576)
    buf = torch.full((n + 4096,), FILL, dtype=torch.int32, device=dev)
    out = torch.full_like(sfe1, float("nan"))
    ptr = lambda t: C.c_void_p(t.data_ptr())                     # noqa: E731
    st = lib.diinn_rdn_forward_ex(C.c_void_p(torch.cuda.current_stream().cuda_stream), N.RDN_ALGO_X3, ptr(sfe1), ptr(packed),
                                  ptr(wino), None, ptr(x3), ptr(biases), ptr(buf), None, ptr(out), b, h, w)
    assert st == 0
    torch.cuda.synchronize()
    return sfe1.cpu(), out.cpu(), buf.cpu()


def _views(buf, shape):
    """The regions of ``planes`` after an X3 forward: the two dense buffers [B,576,H,W], the global-fusion input [B,1024,H,W], the
    64 planes between the two fusion layers, the split buffer as int16 [B,72,2,H*W,8], the guard."""
    b, h, w = shape
    hw = h * w
    f = buf.view(torch.float32)
    o = [0, b * 576 * hw, 2 * b * 576 * hw, b * hw * (2 * 576 + 1024), b * hw * (2 * 576 + 1024 + 64), b * hw * (3 * 576 + 1024 + 64)]
    return (f[o[0]:o[1]].view(b, 576, h, w), f[o[1]:o[2]].view(b, 576, h, w), f[o[2]:o[3]].view(b, 1024, h, w),
            f[o[3]:o[4]].view(b, 64, h, w), buf[o[4]:o[5]].view(torch.int16).view(b, 72, 2, hw, 8), buf[o[5]:])


def _check_split_format(run, shape):
    sfe1, out, buf = run
    b, h, w = shape
    buf0, buf1, gff, _, xs, guard = _views(buf, shape)
    assert guard.numel() == 4096 and bool((guard == FILL).all())
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(gff).all())
    xs_hi, xs_lo = convs.split_planes_decode(xs)                  # [B,576,H*W]
    assert bool(torch.isfinite(xs_hi).all()) and bool(torch.isfinite(xs_lo).all())
    # groups 0..7: block 15's output, written in place by conv1x1_x3_kernel -- the canonical pair of the fp32 planes, bit for bit
    v = buf0[:, :64]
    assert torch.equal(_bits(v), _bits(gff[:, 960:]))
    hi, lo = convs.split_pair(v)
    assert torch.equal(_bits(xs_hi[:, :64]), _bits(hi.reshape(b, 64, h * w)))
    assert torch.equal(_bits(xs_lo[:, :64]), _bits(lo.reshape(b, 64, h * w)))
    # groups 8..71: block 15's dense outputs (after ReLU), each a canonical pair
    d_hi, d_lo = xs_hi[:, 64:], xs_lo[:, 64:]
    assert bool((d_hi >= 0).all())
    assert bool((d_lo[d_hi == 0] == 0).all())
    # (hi is a bf16 nearest to hi + lo: bf16_rne(hi + lo) itself, or -- lo = bf16_rne(v - hi) may round up to exactly half a step of
    # hi, and ties go to even -- the other of two equally near ones)
    s = d_hi + d_lo
    near = s.to(torch.bfloat16).to(torch.float32)
    assert bool(((near == d_hi) | ((s - d_hi).abs() == (s - near).abs())).all())
    assert float((near != d_hi).float().mean()) < 0.02
    assert bool((d_hi > 0).any()) and bool((d_lo != 0).any())
    # in this mode the dense outputs go to the split buffer only
    assert bool((_bits(buf0[:, 64:]) == FILL).all()) and bool((_bits(buf1[:, 64:]) == FILL).all())


def _check_blocks(run, shape, wset, label):
    """Every block (block 0 together with SFENet2 in front of it) and the tail (GFF 1x1 in fp32, GFF 3x3 split, plus sfe1) on the
    kernel's own input against float64, beside the sheet: returns the worst dist_kernel / dist_sheet of the blocks and of the tail."""
    sfe1, out, buf = run
    enc = _encoder(wset)
    gff = _views(buf, shape)[2]
    worst = 0.0
    for d, block in enumerate(enc.RDBs):
        got = gff[:, 64 * d:64 * d + 64]
        if d == 0:
            want = _rdb64(block, _conv64(sfe1.double(), enc.SFENet2))
            x, _, _ = convs.conv_x3_reference(*convs.split_pair(sfe1), enc.SFENet2.weight, enc.SFENet2.bias, 1, relu=False)
        else:
            x = gff[:, 64 * d - 64:64 * d]
            want = _rdb64(block, x.double())
        dk, ds = _dist(got, want), _dist(convs.rdb_x3_reference(block, x)[0], want)
        print(f"{label} block {d}: kernel {dk:.2e} sheet {ds:.2e} ratio {dk / ds:.2f}")
        assert dk <= R * ds, (label, d, dk, ds)
        worst = max(worst, dk / ds)
    want = _conv64(_conv64(gff.double(), enc.GFF[0]), enc.GFF[1]) + sfe1.double()
    t = F.conv2d(gff, enc.GFF[0].weight, enc.GFF[0].bias)
    sheet, _, _ = convs.conv_x3_reference(*convs.split_pair(t), enc.GFF[1].weight, enc.GFF[1].bias, 1, relu=False, residual=sfe1)
    dk, ds = _dist(out, want), _dist(sheet, want)
    print(f"{label} tail: kernel {dk:.2e} sheet {ds:.2e} ratio {dk / ds:.2f}")
    assert dk <= R * ds, (label, "tail", dk, ds)
    return worst, dk / ds


def _check_layers(run, shape, wset, label):
    """Every dense layer of block 15 on the kernel's own inputs: returns the worst dist_kernel / dist_sheet."""
    _, _, buf = run
    b, h, w = shape
    gff, xs = _views(buf, shape)[2], _views(buf, shape)[4]
    xs_hi, xs_lo = convs.split_planes_decode(xs)
    d_hi, d_lo = xs_hi[:, 64:].reshape(b, 512, h, w), xs_lo[:, 64:].reshape(b, 512, h, w)
    got, sheet = _layer_dists(_encoder(wset).RDBs[15], gff[:, 896:960], d_hi, d_lo, sheet=True)
    for c, (dk, ds) in enumerate(zip(got, sheet)):
        print(f"{label} block 15 layer {c}: kernel {dk:.2e} sheet {ds:.2e} ratio {dk / ds:.2f}")
        assert dk <= R * ds, (label, c, dk, ds)
    return max(dk / ds for dk, ds in zip(got, sheet))


def _label(wset, shape, rows):
    return f"{wset} {shape[0]}x{shape[1]}x{shape[2]} rows={rows}"


# kernel forms (DIINN_ENC_X3_ROWS): 0 the launcher's choice (one pixel row per wave on maps this small), 4 the eight-wave
# conv3x3_x3m_kernel, whose accumulators start from the bias (the other forms add it last): other bits, the same rules
FORMS = [0, 4]


@pytest.mark.gpu
@pytest.mark.parametrize("rows", FORMS)
@pytest.mark.parametrize("wset", WSETS)
@pytest.mark.parametrize("shape", MAPS, ids=lambda s: "x".join(map(str, s)))
def test_split_format_after_a_forward(knobs, shape, wset, rows):
    """What the forward leaves in ``planes``: block 15's output in groups 0..7 of the split buffer is bit for bit the pair
    bf16_rne(v), bf16_rne(v - hi) of its fp32 planes (which are the fusion input's last slice); block 15's dense outputs in groups
    8..71 are non-negative canonical pairs; the dense channels of both fp32 buffers and the guard behind ``planes`` were never
    written; nothing is NaN."""
    knobs("DIINN_ENC_X3_MIN", 0)
    knobs("DIINN_ENC_X3_ROWS", rows)
    _check_split_format(_forward_x3(wset, shape, rows), shape)


@pytest.mark.gpu
@pytest.mark.parametrize("rows", FORMS)
@pytest.mark.parametrize("wset", WSETS)
@pytest.mark.parametrize("shape", MAPS, ids=lambda s: "x".join(map(str, s)))
def test_every_block_against_float64(knobs, shape, wset, rows):
    """Each of the 16 blocks and the tail, from the kernel's own fp32 input, against float64: at most R times the sheet's distance
    to the same values (both relative to max|float64 output|).  Measured (MI355X), worst dist_kernel / dist_sheet over the maps,
    default init / gained: blocks 1.13 / 1.21 on the four-wave forms and 1.27 / 1.21 on conv3x3_x3m_kernel, tail 1.13 / 1.07; the
    distances themselves 6e-7 .. 6e-6 (blocks, default init), 1e-6 .. 1e-5 (blocks, gained), 3e-7 .. 6e-6 (tail)."""
    knobs("DIINN_ENC_X3_MIN", 0)
    knobs("DIINN_ENC_X3_ROWS", rows)
    _check_blocks(_forward_x3(wset, shape, rows), shape, wset, _label(wset, shape, rows))


@pytest.mark.gpu
@pytest.mark.parametrize("rows", FORMS)
@pytest.mark.parametrize("wset", WSETS)
@pytest.mark.parametrize("shape", MAPS, ids=lambda s: "x".join(map(str, s)))
def test_every_dense_layer_of_the_last_block_against_float64(knobs, shape, wset, rows):
    """Block 15 has all eight Cin values (64 .. 512) the kernels ever see: layer c, read from groups 8 (c + 1) .. 8 (c + 1) + 7 as
    hi + lo, against float64 ReLU(conv) of the kernel's own inputs (the fusion input's slice 14, the stored pairs of the layers
    before it): at most R times the sheet's distance.  Measured (MI355X): both distances are the rounding of the stored pair,
    3e-6 .. 1.1e-5 of max|out|, and equal on most layers (ratio 1.00); where the kernel's fp32 sum differs in its last bits a lo
    half rounds the other way at the worst element: worst dist_kernel / dist_sheet 1.67 (default init, 1 x 5 x 3, four-wave forms),
    1.51 on conv3x3_x3m_kernel; gained 1.07 / 1.43."""
    knobs("DIINN_ENC_X3_MIN", 0)
    knobs("DIINN_ENC_X3_ROWS", rows)
    _check_layers(_forward_x3(wset, shape, rows), shape, wset, _label(wset, shape, rows))


@pytest.mark.gpu
@pytest.mark.parametrize("wset", WSETS)
@pytest.mark.parametrize("shape", MAPS, ids=lambda s: "x".join(map(str, s)))
def test_four_wave_kernel_forms_are_bit_equal(knobs, shape, wset):
    """DIINN_ENC_X3_ROWS = 1 (one pixel row per wave), 2 (two rows, weight ring) and 3 (two rows, a group's weights ahead in
    registers) issue the same products in the same order per accumulator and add the bias last: on the MI355X the whole ``planes``
    buffer and the features are bit-equal between them and with the launcher's own choice (0), so the three tests above hold for
    all of them; form 4 differs in bits (features 2e-7 .. 9e-7 of max|feat| away at default init) and runs them itself."""
    knobs("DIINN_ENC_X3_MIN", 0)
    knobs("DIINN_ENC_X3_ROWS", 0)
    _, out0, buf0 = _forward_x3(wset, shape, 0)
    for rows in (1, 2, 3):
        _, out, buf = _forward_x3(wset, shape, rows)
        assert torch.equal(buf, buf0) and torch.equal(_bits(out), _bits(out0)), rows


@pytest.mark.gpu
def test_split_bf16_dispatch_threshold():
    """At default knobs the split-bf16 layers start at 32,768 pixels: with hip_split_bf16 set, 127 x 256 returns the fp32 trunk's
    features bit for bit (F(2x2) layers, which is where DIINN_RDN_ALGO_X3 falls back to), 128 x 256 other bits within 3e-5 of
    max|feat| (the bound of test_trunk_with_split_bf16_layers_tracks_the_fp32_trunk)."""
    enc = _device_encoder("default")
    dev = torch.device("cuda:0")
    try:
        with torch.no_grad():
            for h, split in ((127, False), (128, True)):
                assert convs.conv_form(1, h, 256) == "wino"
                x = _image(1, h, 256).to(dev)
                enc.hip_split_bf16 = False
                f32 = enc(x)
                enc.hip_split_bf16 = True
                f3 = enc(x)
                assert bool(torch.isfinite(f3).all())
                assert torch.equal(f3, f32) != split, h
                assert float((f3 - f32).abs().max()) <= 3e-5 * float(f32.abs().max()), h
    finally:
        enc.hip_split_bf16 = False
