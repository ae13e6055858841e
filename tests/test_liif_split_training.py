"""LIIF under autograd in split-bf16 arithmetic (``LIIF.hip_autograd_split_bf16``; diinn_amd.liif_split_training), without a GPU:
the emulation sheet against the float64 oracle (pre-activations, gates, the backward chain, the gradients with pinned gates), the
backward half of the split training image, the switch and its refusals, the symbols.  The library is needed for the axis tables
and the host packer only.  tests/test_liif_split_training_gpu.py holds the kernels against the same sheets.

Shapes are (B, H, W, Hu, Wu, gain): the five reference fixtures of tests/test_liif_training.py (their own seeds) and five shapes
chosen for the plane tiling over the virtual pixels (seed 123; gain3: seed 140, see SEEDS)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import diinn_amd.synth as synth

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = ["b2_3x2_5x4", "b1_4x3_9x7", "b1_8x8_5x6_down", "b1_1x1_7x5", "b1_2x3_8x12_gain2"]
SHAPES = {                                   # (B, H, W, Hu, Wu, gain)
    "px1": (1, 1, 1, 1, 1, 1.0),             # 4 virtual pixels: every tile is ragged, all four members share one tile
    "9x4": (1, 3, 2, 9, 4, 1.0),             # N = 36, 4.5 tiles: member borders mid-tile, the second forward wave is ragged
    "n96": (1, 4, 3, 8, 12, 1.0),            # 384 virtual pixels: whole tiles and whole workgroups only, member borders tile-aligned
    "gain3": (1, 3, 2, 9, 4, 3.0),           # large activations: the worst case for the split rounding
    "b2_12x10_31x27": (2, 12, 10, 31, 27, 1.0),   # 209.25 tiles, 7.5 cell tiles: the shape of the existing mask test
}
# Seed 123 except gain3.  The gate caps below are conditions on the INPUTS, and at gain 3 seed 123 does not meet one: its smallest
# float64 pre-activation of layer 4 (2.2e-5) lies at 0.23 x the sheet's own distance from float64 in that layer (9.5e-5), inside
# the split rounding, so the sign the arithmetic gives it is an accident of the summation order (the sheet keeps it, the kernel's
# order does not).  140 is the first seed from 123 on at which every pre-activation of layers 2..4 is at least twice the sheet's
# largest error of its layer away from zero (6.1, 2.5, 2.3 x); test_input_condition_of_gain3 asserts it, from the sheet and the
# oracle alone.
SEEDS = {"gain3": 140}
ALL = FIXTURES + list(SHAPES)
BIG = "b2_12x10_31x27"
PNAMES = [f"layers.{i}.{t}" for i in (0, 2, 4, 6, 8) for t in ("weight", "bias")]
IMNET_SHAPES = {"imnet.layers.0.weight": (256, 580), "imnet.layers.0.bias": (256,),
                **{f"imnet.layers.{i}.weight": (256, 256) for i in (2, 4, 6)}, **{f"imnet.layers.{i}.bias": (256,) for i in (2, 4, 6)},
                "imnet.layers.8.weight": (3, 256), "imnet.layers.8.bias": (3,)}
RTOL = 1e-4                                  # the project's gradient bound (tests/test_liif_training.py)
ATOL = 1e-4                                  # the forward contract: 1e-4 x max(1, max|a_64|)


def gate_cap(name, n):
    """Gates of layers 2..4 that may differ from float64's: a condition on the inputs, not on the code."""
    return math.ceil(1e-5 * 3 * 256 * 4 * n) if name == BIG else 0


_cases = {}


def case(name):
    """(ws [ten arrays, PNAMES order], feat, gout, (b, h, w, hu, wu)) of a shape; built once."""
    if name not in _cases:
        if name in SHAPES:
            b, h, w, hu, wu, gain = SHAPES[name]
            seed = SEEDS.get(name, 123)
        else:
            meta = np.load(os.path.join(HERE, "golden", f"liif_golden_grad_{name}.npz"))["meta"]
            b, h, w, hu, wu, gain, seed = [int(v) for v in meta[:5]] + [float(meta[5]), int(meta[6])]
        sd = synth.state_dict_for(IMNET_SHAPES, seed, "liif.", gain=gain)
        _cases[name] = ([sd["imnet." + n] for n in PNAMES], synth.encoder_features(seed, b, h, w),
                        synth.uniform(seed, f"gradw:liif:{name}", (b, 3, hu, wu), 1.0), (b, h, w, hu, wu))
    return _cases[name]


_sheets = {}


def sheets(name):
    """Per shape, computed once on the CPU and left unchanged: (a_x3 [4 x [4,N,256]] fp32 from the emulation sheet, a_64 the float64
    oracle's pre-activations)."""
    if name not in _sheets:
        import diinn_amd.liif_split_training as LS
        import diinn_amd.liif_training as LT
        ws, feat, _r, (b, h, w, hu, wu) = case(name)
        p32 = [torch.from_numpy(x) for x in ws]
        a_x3 = LS.liif_split_preactivations(torch.from_numpy(feat), p32, (hu, wu))
        a_64 = LT.liif_preactivations(torch.from_numpy(feat).double(), [p.double() for p in p32], (hu, wu))
        _sheets[name] = (a_x3, a_64)
    return _sheets[name]


def test_shape_table_is_the_issues():
    b, h, w, hu, wu, _ = SHAPES["px1"]
    assert 4 * b * hu * wu == 4
    b, h, w, hu, wu, _ = SHAPES["9x4"]
    assert b * hu * wu == 36 and (4 * 36) % 32 == 16
    b, h, w, hu, wu, _ = SHAPES["n96"]
    assert 4 * b * hu * wu == 384 and (b * hu * wu) % 32 == 0
    b, h, w, hu, wu, _ = SHAPES[BIG]
    assert 4 * b * hu * wu == 209 * 32 + 8 and gate_cap(BIG, b * hu * wu) == 52
    assert len(ALL) == 10


def test_input_condition_of_gain3():
    """Every float64 pre-activation of layers 2..4 of gain3 is at least twice the emulation sheet's largest distance from float64
    in its layer away from zero (see SEEDS): no gate of this shape hangs on the summation order of the split products."""
    a_x3, a_64 = sheets("gain3")
    for l in (1, 2, 3):
        noise = float((a_x3[l].double() - a_64[l]).abs().max())
        assert float(a_64[l].abs().min()) >= 2.0 * noise, (l, float(a_64[l].abs().min()), noise)


@pytest.mark.parametrize("name", ALL)
def test_emulation_sheet_against_the_oracle(name):
    """``liif_split_preactivations`` against ``liif_preactivations`` in float64: max|relu(a_x3) - relu(a_64)| <= 1e-4 x max(1, max|a_64|)
    per layer (measured with the sheet: at most 1.0e-5, on gain3).  Gates of layers 2..4 that differ from float64's: at most
    ceil(1e-5 x 3 x 256 x 4 N) = 52 on b2_12x10_31x27 (measured 12; the fp32 formula sheet has 2), exactly 0 on the other nine -- these
    counts are conditions on the inputs: if a seed change ever breaks them, choose another seed, do not widen the cap."""
    a_x3, a_64 = sheets(name)
    ws, feat, _r, (b, h, w, hu, wu) = case(name)
    n = b * hu * wu
    assert len(a_x3) == 4 and all(tuple(a.shape) == (4, n, 256) and a.dtype == torch.float32 for a in a_x3)
    differ = 0
    for l in range(4):
        err = float((torch.relu(a_x3[l]).double() - torch.relu(a_64[l])).abs().max())
        bound = ATOL * max(1.0, float(a_64[l].abs().max()))
        d = int(((a_x3[l] > 0) != (a_64[l] > 0)).sum())
        print(f"liif split sheet {name} layer {l + 1}: max|relu(a_x3) - relu(a_64)| = {err:.3e} (bound {bound:.3e}), {d} gates differ")
        assert err <= bound, (name, l, err)
        if l == 0:
            assert d == 0, (name, d)                                # layer 1 is fp32 in the sheet as in the kernel
        else:
            differ += d
    print(f"liif split sheet {name}: {differ} gates of layers 2..4 differ from float64's (cap {gate_cap(name, n)})")
    assert differ <= gate_cap(name, n), (name, differ)


def chains(name):
    """(hs fp32 = relu of the sheet's pre-activations, the sheet's chain fp32, the float64 chain on the same hs)."""
    import diinn_amd.liif_split_training as LS
    ws, feat, r, (b, h, w, hu, wu) = case(name)
    hs = [torch.relu(a) for a in sheets(name)[0]]
    p32 = [torch.from_numpy(x) for x in ws]
    c32 = LS.liif_split_chain_reference(torch.from_numpy(r), hs, p32, (h, w))
    c64 = LS.liif_split_chain_reference(torch.from_numpy(r).double(), [x.double() for x in hs], [p.double() for p in p32], (h, w), split=False)
    return hs, c32, c64


@pytest.mark.parametrize("name", ALL)
def test_sheet_of_the_backward_chain(name):
    """``liif_split_chain_reference`` against the float64 chain on the same ``hs`` and therefore the same gates: per plane
    <= 1e-4 x max|ref| (measured with the sheet: at most 9.8e-6)."""
    hs, c32, c64 = chains(name)
    assert len(c32) == 4 and all(c.dtype == torch.float32 and c.shape == hs[0].shape for c in c32)
    for i, (g32, g64) in enumerate(zip(c32, c64)):
        err, scale = float((g32.double() - g64).abs().max()), float(g64.abs().max())
        print(f"liif split chain sheet {name} g_a,{4 - i}: err {err:.3e} = {err / max(scale, 1e-30):.2e} max|ref| ({scale:.3e})")
        assert err <= RTOL * scale, (name, 4 - i, err, scale)
        assert torch.equal(g32 != 0, (g32 != 0) & (hs[3 - i] > 0))     # a closed gate is an exact zero


@pytest.mark.parametrize("name", ALL)
def test_sheet_gradients_with_pinned_gates(name):
    """The ten parameter gradients and d feat from ``liif_backward_from_saved`` fed the sheet's chain (fp32), against the same
    function in float64 on the same ``hs``: <= 1e-4 x max|ref| per tensor.  The per-tensor figures are printed."""
    import diinn_amd.liif_split_training as LS
    ws, feat, r, (b, h, w, hu, wu) = case(name)
    hs, c32, _c64 = chains(name)
    p32 = [torch.from_numpy(x) for x in ws]
    d32, g32 = LS.liif_backward_from_saved(torch.from_numpy(r), torch.from_numpy(feat), hs, p32, (hu, wu), chain=c32)
    d64, g64 = LS.liif_backward_from_saved(torch.from_numpy(r).double(), torch.from_numpy(feat).double(), [x.double() for x in hs],
                                           [p.double() for p in p32], (hu, wu))
    assert d32.dtype == torch.float32 and d64.dtype == torch.float64 and tuple(d32.shape) == feat.shape
    for pname, got, ref in zip(["feat"] + PNAMES, [d32] + g32, [d64] + g64):
        assert got.shape == ref.shape, pname
        err, scale = float((got.double() - ref).abs().max()), float(ref.abs().max())
        print(f"liif split sheet grads {name} {pname}: err {err:.3e} = {err / max(scale, 1e-30):.2e} max|ref| ({scale:.3e})")
        assert err <= RTOL * scale, (name, pname, err, scale)
    none, _ = LS.liif_backward_from_saved(torch.from_numpy(r), torch.from_numpy(feat), hs, p32, (hu, wu), need_feat_grad=False, chain=c32)
    assert none is None


def test_from_saved_on_the_oracles_own_activations_is_the_formula_sheet():
    """``liif_backward_from_saved`` on relu of the float64 pre-activations reproduces ``liif_backward_reference`` in float64."""
    import diinn_amd.liif_split_training as LS
    import diinn_amd.liif_training as LT
    ws, feat, r, (b, h, w, hu, wu) = case("b1_4x3_9x7")
    p64 = [torch.from_numpy(x).double() for x in ws]
    f64, r64 = torch.from_numpy(feat).double(), torch.from_numpy(r).double()
    hs = [torch.relu(a) for a in LT.liif_preactivations(f64, p64, (hu, wu))]
    d_a, g_a = LS.liif_backward_from_saved(r64, f64, hs, p64, (hu, wu))
    d_b, g_b = LT.liif_backward_reference(r64, f64, p64, (hu, wu))
    for x, y in zip([d_a] + g_a, [d_b] + g_b):
        assert float((x - y).abs().max()) <= 1e-12 * max(1.0, float(y.abs().max()))


def test_backward_half_of_the_split_image():
    """The backward half of ``pack_liif_split(pack_liif_state_dict(sd))`` -- [layer 3][m 8][ks 16][piece 4][lane 64][j 8] bf16
    (diinn_layout.h) -- holds zero bytes in pieces 0 and 2 and, in pieces 1 / 3, hi / lo of W^T at
    [out = chan_of_bf16(ks, lane >> 5, j)][in = 32 m + (lane & 31)] for imnet.layers.{2,4,6}: the twin of the forward-half test of
    tests/test_liif_x3.py.  This is what liif_bwd_layer_x3_kernel streams."""
    import diinn_amd._native as N
    import diinn_amd.decoder as D
    import diinn_amd.sheets as S
    sd = synth.state_dict_for(IMNET_SHAPES, 123, "liif.", gain=2.0)
    split = D.pack_liif_split(D.pack_liif_state_dict(sd))
    assert split.dtype == torch.float32 and split.numel() == N.load().diinn_split_train_floats()
    half = split.numel() // 2
    bwd = split.numpy()[half:].view(np.uint16).reshape(3, 8, 16, 4, 64, 8)
    assert not bwd[:, :, :, 0].any() and not bwd[:, :, :, 2].any()
    lane, j = np.arange(64)[:, None], np.arange(8)[None, :]
    for layer, name in enumerate(("imnet.layers.2.weight", "imnet.layers.4.weight", "imnet.layers.6.weight")):
        hi, lo = S.split_hi_lo(torch.from_numpy(sd[name]))
        hi16 = (hi.numpy().view(np.uint32) >> 16).astype(np.uint16)
        lo16 = (lo.numpy().view(np.uint32) >> 16).astype(np.uint16)
        for m in range(8):
            for ks in range(16):
                in_ch = np.broadcast_to(32 * m + (lane & 31), (64, 8))
                out_ch = 32 * (ks >> 1) + 16 * (ks & 1) + 8 * (j >> 2) + 4 * (lane >> 5) + (j & 3)     # chan_of_bf16(ks, lane >> 5, j)
                assert np.array_equal(bwd[layer, m, ks, 1], hi16[out_ch, in_ch]), (name, m, ks, "hi")
                assert np.array_equal(bwd[layer, m, ks, 3], lo16[out_ch, in_ch]), (name, m, ks, "lo")


def test_switch_and_refusals_without_a_gpu():
    """``hip_autograd_split_bf16``: a plain attribute and constructor keyword, default False, not in the state dict, left alone by
    ``set_split_bf16``.  It acts only together with ``hip_autograd`` and ``hip_split_bf16``: with all three set a CPU tensor under
    grad reaches "the training forward runs on a ROCm GPU only"; with the new switch off the fp32-only refusal stays word for
    word; with ``hip_autograd`` off the opt-in refusal stays word for word; with ``hip_split_bf16`` off it changes nothing (the fp32
    training forward's device check); with ``bsize`` the no_grad decode."""
    import diinn_amd.modules as M
    assert M.LIIF.hip_autograd_split_bf16 is False
    net = M.LIIF()
    assert net.hip_autograd_split_bf16 is False and "hip_autograd_split_bf16" not in net.state_dict()
    on = M.LIIF(hip_autograd=True, hip_split_bf16=True, hip_autograd_split_bf16=True)
    assert on.hip_autograd_split_bf16 is True and on.hip_split_bf16 is True and on.hip_autograd is True
    assert "hip_autograd_split_bf16" not in on.state_dict() and "hip_autograd_split_bf16" not in dict(on.named_buffers())
    assert net.set_split_bf16() is net and net.hip_split_bf16 is True and net.hip_autograd_split_bf16 is False
    assert on.set_split_bf16(False) is on and on.hip_split_bf16 is False and on.hip_autograd_split_bf16 is True
    on.set_split_bf16(True)
    on.encoder.hip_split_bf16 = False
    assert on.hip_autograd_split_bf16 is True
    x = torch.zeros(1, 3, 4, 4)
    with pytest.raises(RuntimeError) as e:                            # all three: past every refusal, to the device check
        on(x, (8, 8))
    assert str(e.value) == "diinn_amd: the training forward runs on a ROCm GPU only (no CPU implementation)"
    fp32_only = ("diinn_amd: LIIF trains in fp32 only: unset LIIF.hip_split_bf16 (the split-bf16 "
                 "decoder is inference-only), or call under torch.no_grad()")
    on.hip_autograd_split_bf16 = False                                # the new switch off: the refusal that was there
    with pytest.raises(NotImplementedError) as e:
        on(x, (8, 8))
    assert str(e.value) == fp32_only
    on.hip_autograd_split_bf16 = True
    on.hip_autograd = False                                           # hip_autograd off: the opt-in refusal
    opt_in = ("diinn_amd: LIIF under autograd is opt-in: set LIIF.hip_autograd = True (the decoder then trains "
              "on the HIP kernels), or call under torch.no_grad()")
    with pytest.raises(NotImplementedError) as e:
        on(x, (8, 8))
    assert str(e.value) == opt_in
    on.hip_autograd = True
    on.hip_split_bf16 = False                                         # hip_split_bf16 off: fp32 training as today
    with pytest.raises(RuntimeError, match="the training forward runs on a ROCm GPU only"):
        on(x, (8, 8))
    on.hip_split_bf16 = True
    with pytest.raises(RuntimeError, match="ROCm GPU"):               # bsize given: the no_grad decode
        on(x, (8, 8), 300)
    with torch.no_grad(), pytest.raises(RuntimeError, match="ROCm GPU"):
        on(x, (8, 8))


def test_symbols_are_declared_exported_and_bound(tmp_path):
    """``diinn_liif_train_fwd_x3`` and ``diinn_liif_backward_data_x3`` in the header, the library and ``SIGNATURES`` (one pointer more
    than their fp32 twins); ABI 11.  Where llvm-readelf is installed: the training forward and both instantiations of the backward
    kernel are in the library without scratch, dynamic stack or VGPR spills at one wave per SIMD or better, and the backward uses
    no LDS."""
    import diinn_amd._native as N
    import test_kernel_resources as K
    header = open(os.path.join(HERE, "..", "include", "diinn_hip.h")).read()
    lib = C.CDLL(N.LIB_PATH)
    for sym, twin in (("diinn_liif_train_fwd_x3", "diinn_liif_train_fwd"), ("diinn_liif_backward_data_x3", "diinn_liif_backward_data")):
        assert re.search(r"^int\s+" + sym + r"\s*\(", header, re.M), sym
        assert hasattr(lib, sym) and sym in N.SIGNATURES, sym
        assert len(N.SIGNATURES[sym][1]) == len(N.SIGNATURES[twin][1]) + 1
    assert N.load().diinn_abi_version() == 11
    if not os.path.exists(K.READELF):
        return
    ks = K.kernel_metadata(N.LIB_PATH, tmp_path)
    fwd = [k for k in ks if K.base_name(k[".name"]) == "liif_x3_save_kernel"]
    bwd = [k for k in ks if K.base_name(k[".name"]) == "liif_bwd_layer_x3_kernel"]
    assert len(fwd) == 1 and len(bwd) == 2
    for k in fwd + bwd:
        assert int(k[".private_segment_fixed_size"]) == 0 and not k.get(".uses_dynamic_stack") and int(k[".vgpr_spill_count"]) == 0
        assert K.occupancy(k) >= 1
    assert all(int(k[".group_segment_fixed_size"]) == 0 for k in bwd)
    inference = [k for k in ks if K.base_name(k[".name"]) == "liif_x3_kernel"]
    assert len(inference) == 1 and int(fwd[0][".group_segment_fixed_size"]) == int(inference[0][".group_segment_fixed_size"])
