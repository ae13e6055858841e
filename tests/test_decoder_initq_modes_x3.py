"""Decoder ``init_q=True`` with modes 1, 2 and 4 in split-bf16 arithmetic (``compute="bf16x3"`` behind
``ImplicitDecoder.hip_initq_modes`` + ``hip_initq_modes_split_bf16`` / ``decode_features_initq(compute="bf16x3", initq_x3=...)``):
``initq_planes_x3_kernel`` (mode 1: its 512-row form), ``pixel_chain_x3_kernel`` with ``decode_bf16x3_kernel<SIN | X3_INITQ | X3_QONLY>``
(modes 1/2), ``decode_bf16x3_kernel<SIN | X3_INITQ | X3_TAPS>`` with the unchanged gather (mode 4), the C ABI entry points
``diinn_decode_initq_mode{1,2,4}_x3`` and the emulation sheet ``decoder.initq_modes_x3_forward_reference``.

Fixtures: tests/golden/diinn_golden_initq_modes.npz, the real reference in fp32 and its distance to the reference's float64 run (the
21 cases of tests/test_decoder_initq_modes.py).  Contract everywhere: ``1e-4 x max(1, max|ref32|)`` of the case (= 1e-4 on every
case).  The accurate sine is held to the noise-floor bound as well: ``max|hip - ref64| <= FACTOR x N'`` with N' the largest
``max|emulation - ref64|`` over the cases of the same mode and gain and FACTOR = 3.0, the project's noise-floor factor."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import diinn_amd.synth as synth

gpu = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
TOL = 1e-4
FACTOR = 3.0
MODES = (1, 2, 4)
NAMES = ["c1x1_2x2", "row1x9_2x30", "b3_7x5_23x18", "b2_12x10_31x27_gain2", "down16x12_8x6", "small4x3_110x9", "siren_9x14_36x56"]
GAIN2 = "b2_12x10_31x27_gain2"
NEW_SYMBOLS = ("diinn_initq_planes_m1_x3", "diinn_pixel_chain_x3", "diinn_decode_initq_mode1_x3", "diinn_decode_initq_mode2_x3",
               "diinn_decode_initq_mode4_x3")
CANARY = -7.25


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(HERE, "golden", "diinn_golden_initq_modes.npz"))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return torch.device("cuda:0")


def _case(g, mode, name):
    b, h, w, hu, wu, gain, fgain = g[f"meta/{mode}/{name}"]
    return int(b), int(h), int(w), int(hu), int(wu), float(gain), float(fgain)


def _refs(g, mode, name):
    ref32 = g[f"out/{mode}/{name}"]
    return ref32, ref32.astype(np.float64) + g[f"d64/{mode}/{name}"].astype(np.float64)


def _state_dict(mode, gain=1.0, fgain=1.0, seed=123):
    sd = synth.decoder_state_dict(seed, gain, mode=mode, init_q=True)
    sd["first_layer.0.weight"] = (sd["first_layer.0.weight"] * np.float32(fgain)).astype(np.float32)
    return sd


def _tol(ref):
    return TOL * max(1.0, float(np.abs(ref).max()))


_EMUL = {}


def _emulation(g, mode, name):
    """The emulation sheet of one fixture case on the CPU, computed once per session and shared (never modified)."""
    import diinn_amd.decoder as D
    if (mode, name) not in _EMUL:
        b, h, w, hu, wu, gain, fgain = _case(g, mode, name)
        feat = torch.from_numpy(synth.encoder_features(123, b, h, w))
        em = D.initq_modes_x3_forward_reference(_state_dict(mode, gain, fgain), feat, (hu, wu), mode).numpy()
        em.setflags(write=False)
        _EMUL[(mode, name)] = em
    return _EMUL[(mode, name)]


def _noise(g, mode):
    """N' per gain: the largest max|emulation - ref64| over the cases of that mode and gain."""
    n = {}
    for name in NAMES:
        gain = _case(g, mode, name)[5]
        n[gain] = max(n.get(gain, 0.0), float(np.abs(_emulation(g, mode, name) - _refs(g, mode, name)[1]).max()))
    return n


def _module(mode, sd, dev=None, **kw):
    import diinn_amd.decoder as D
    kw = {"hip_initq_modes": True, "hip_initq_modes_split_bf16": True, "compute": "bf16x3", **kw}
    dec = D.ImplicitDecoder(mode=mode, init_q=True, **kw)
    dec.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    return (dec.to(dev) if dev is not None else dec).eval()


def _images(sd, mode, dev):
    import diinn_amd.decoder as D
    packed = D.pack_state_dict(D.initq_body_state_dict(sd), mode=mode).to(dev)
    head = D.pack_head3x3(sd).to(dev) if mode == 4 else None
    return packed, D.pack_initq(sd).to(dev), D.pack_initq_x3(sd).to(dev), head


def _decode_x3(feat, images, size, mode, **kw):
    import diinn_amd.decoder as D
    packed, image, image_x3, head = images
    return D.decode_features_initq(feat, packed, image, size, mode, head=head, compute="bf16x3", initq_x3=image_x3, **kw)


def _ptr(t):
    return C.c_void_p(None if t is None else t.data_ptr())


# ---------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_the_switch_opens_the_combination_and_nothing_else(mode):
    """Fails on the parent commit: there the constructor and ``decode_features_initq`` have no such keywords.  The switch is a plain
    attribute and constructor keyword, default False, untouched by ``DIINN.set_split_bf16()``.  With ``hip_initq_modes``,
    ``compute="bf16x3"`` and the switch set, a CPU tensor under no_grad (and with ``bsize`` given) has passed every refusal and
    reaches the device check; so does the functional entry.  With the switch off the refusal is the one it was."""
    import diinn_amd.decoder as D
    import diinn_amd.modules as M
    x = torch.zeros(1, 64, 4, 4)                      # CPU tensors: a refusal that looked at the device would raise RuntimeError
    img = torch.zeros(4)
    assert D.ImplicitDecoder.hip_initq_modes_split_bf16 is False
    assert D.ImplicitDecoder(mode=mode, init_q=True).hip_initq_modes_split_bf16 is False
    on = D.ImplicitDecoder(mode=mode, init_q=True, compute="bf16x3", hip_initq_modes=True, hip_initq_modes_split_bf16=True)
    assert on.hip_initq_modes_split_bf16 is True
    with torch.no_grad(), pytest.raises(RuntimeError, match="ROCm GPU"):
        on(x, (8, 8))
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        on(x, (8, 8), 30000)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        D.decode_features_initq(x, img, img, (8, 8), mode, head=img, compute="bf16x3", initq_x3=img)
    net = M.DIINN(mode=mode, init_q=True)
    net.set_split_bf16()
    assert net.decoder.compute == "bf16x3" and net.decoder.hip_initq_modes_split_bf16 is False
    net.decoder.hip_initq_modes = True
    with torch.no_grad(), pytest.raises(ValueError, match="fp32 only"):
        net.decoder(x, (8, 8), 30000)
    net.decoder.hip_initq_modes_split_bf16 = True     # the second line a user writes
    with torch.no_grad(), pytest.raises(RuntimeError, match="ROCm GPU"):
        net.decoder(x, (8, 8), 30000)
    # the switch off, or on without hip_initq_modes: as before
    for kw in ({"hip_initq_modes": True}, {"hip_initq_modes": True, "hip_initq_modes_split_bf16": False},
               {"hip_initq_modes": True, "hip_initq_split_bf16": True, "hip_modes_split_bf16": True}):
        with torch.no_grad(), pytest.raises(ValueError, match="fp32 only"):
            D.ImplicitDecoder(mode=mode, init_q=True, compute="bf16x3", **kw)(x, (8, 8))
    with torch.no_grad(), pytest.raises(NotImplementedError, match="mode 3"):
        D.ImplicitDecoder(mode=mode, init_q=True, compute="bf16x3", hip_initq_modes_split_bf16=True)(x, (8, 8))
    # fp32 gives what it gave, whatever is set
    with torch.no_grad(), pytest.raises(RuntimeError, match="ROCm GPU"):
        D.ImplicitDecoder(mode=mode, init_q=True, hip_initq_modes=True, hip_initq_modes_split_bf16=True)(x, (8, 8))


@pytest.mark.parametrize("mode", MODES)
def test_what_keeps_refusing_with_everything_on(mode):
    import diinn_amd.decoder as D
    import diinn_amd.modules as M
    x = torch.zeros(1, 64, 4, 4)
    img = torch.zeros(4)
    every = {"hip_initq_modes": True, "hip_initq_modes_split_bf16": True, "hip_autograd": True, "hip_autograd_mode4": True,
             "hip_autograd_initq_modes": True, "hip_initq_split_bf16": True, "hip_autograd_initq_split_bf16": True,
             "hip_autograd_split_bf16": True, "hip_modes_split_bf16": True}
    dec = D.ImplicitDecoder(mode=mode, init_q=True, compute="bf16x3", **every)
    with pytest.raises(NotImplementedError):          # autograd with bsize=None
        dec(x, (8, 8))
    with pytest.raises(NotImplementedError):
        dec.requires_grad_(False)(x.clone().requires_grad_(True), (8, 8))
    for comp in ("bf16", "bf16_full"):
        with torch.no_grad(), pytest.raises(ValueError, match="fp32 only"):
            D.ImplicitDecoder(mode=mode, init_q=True, compute=comp, **every)(x, (8, 8))
        with pytest.raises(ValueError, match="'f32' or 'bf16x3'"):
            D.decode_features_initq(x, img, img, (8, 8), mode, head=img, compute=comp, initq_x3=img)
    with pytest.raises(ValueError, match="initq_x3"):
        D.decode_features_initq(x, img, img, (8, 8), mode, head=img, compute="bf16x3")
    with pytest.raises(ValueError, match="initq_x3"):
        D.decode_features_initq(x, img, img, (8, 8), mode, head=img, initq_x3=img)
    with pytest.raises(NotImplementedError, match="graphs"):
        M.DIINN(mode=mode, init_q=True, graphs=True)
    net = M.DIINN(mode=mode, init_q=True)
    net.set_split_bf16()
    net.decoder.hip_initq_modes = net.decoder.hip_initq_modes_split_bf16 = True
    with pytest.raises(NotImplementedError, match="mode 4" if mode == 4 else "init_q"):
        net.forward_sharded(torch.zeros(1, 3, 4, 4), (8, 8))
    with pytest.raises(ValueError, match="modes 1, 2 and 4"):
        D.initq_modes_x3_forward_reference({}, x, (8, 8), 3)


@pytest.mark.parametrize("mode", MODES)
def test_emulation_sheet_meets_the_contract_and_the_fixture_can_fail(gold, mode, monkeypatch):
    """``initq_modes_x3_forward_reference`` against ref32 of every case: within the contract.  Expected near 3.9e-6 at worst (mode 2,
    the gain-2 case) and <= 1e-7 on gain-1 cases; the host's matmul may move the last digit.  With ``split_matmul`` replaced by a
    two-product form (either small product omitted) the sheet EXCEEDS the contract on the gain-2 case: a dropped product does not
    pass this fixture."""
    import diinn_amd.decoder as D
    import diinn_amd.sheets as S
    for name in NAMES:
        ref32, _ = _refs(gold, mode, name)
        em = _emulation(gold, mode, name)
        assert em.shape == ref32.shape and em.dtype == np.float32
        err = float(np.abs(em - ref32).max())
        print(f"mode {mode} {name}: max|emulation - ref32| = {err:.3e} / {_tol(ref32):.3e}")
        assert err <= _tol(ref32), f"mode {mode} {name}: {err:.3e} > {_tol(ref32):.3e}"
    b, h, w, hu, wu, gain, fgain = _case(gold, mode, GAIN2)
    sd = _state_dict(mode, gain, fgain)
    feat = torch.from_numpy(synth.encoder_features(123, b, h, w))
    ref32, _ = _refs(gold, mode, GAIN2)
    for drop in (0, 1):
        def two_products(w_, q_, drop=drop):
            wh, wl = S.split_hi_lo(w_)
            qh, ql = S.split_hi_lo(q_)
            return (wh @ ql if drop == 0 else wl @ qh) + wh @ qh
        monkeypatch.setattr(S, "split_matmul", two_products)
        bad = D.initq_modes_x3_forward_reference(sd, feat, (hu, wu), mode).numpy()
        monkeypatch.undo()
        err = float(np.abs(bad - ref32).max())
        print(f"mode {mode} {GAIN2}: without {('w_lo.x_hi', 'w_hi.x_lo')[drop]}: {err:.3e} / {_tol(ref32):.3e}")
        assert err > _tol(ref32), (mode, drop, err)


def test_entry_points_validate_before_they_touch_a_device():
    """Declared in the header, exported, bound; ABI version 11.  Null pointers, a misaligned ``pix`` or image, a bad band, a bad
    sine mode: refused with a status, nothing launched (no device is present on the build host)."""
    import diinn_amd._native as N
    lib = N.load()
    assert lib.diinn_abi_version() == 11 == N.ABI_VERSION
    header = open(os.path.join(os.path.dirname(HERE), "include", "diinn_hip.h")).read()
    for sym in NEW_SYMBOLS:
        assert sym + "(" in header, sym
        assert sym in N.SIGNATURES and getattr(lib, sym).argtypes == N.SIGNATURES[sym][1], sym
    one, odd = C.c_void_p(16), C.c_void_p(8)
    dims, band = (1, 4, 4, 8, 8), (0, 8)
    E, U = N.ERR_INVALID_ARG, N.ERR_UNSUPPORTED
    # the 512-row planes form: diinn_initq_planes_x3's checks
    f = lib.diinn_initq_planes_m1_x3
    good = [one] * 5
    for i in range(5):
        assert f(None, *[None if j == i else p for j, p in enumerate(good)], *dims, *band, 0) == E, i
    assert f(None, *good, *dims, 4, 4, 0) == E
    assert f(None, *good, *dims, 0, 9, 0) == E
    assert f(None, *good, *dims, *band, 7) == U
    # modes 1/2: feat, packed, initq, initq_x3, pix, out
    for f in (lib.diinn_decode_initq_mode1_x3, lib.diinn_decode_initq_mode2_x3):
        good = [one] * 6
        for i in range(6):
            assert f(None, *[None if j == i else p for j, p in enumerate(good)], *dims, *band, 0) == E, i
        for i in (1, 2, 3, 4):                                     # the images and pix: 16-byte aligned
            assert f(None, *[odd if j == i else p for j, p in enumerate(good)], *dims, *band, 0) == E, i
        assert f(None, *good, *dims, 8, 8, 0) == E
        assert f(None, *good, *dims, -1, 4, 0) == E
        assert f(None, *good, *dims, 0, 9, 0) == E
        assert f(None, *good, 0, 4, 4, 8, 8, *band, 0) == E
        assert f(None, *good, *dims, *band, 3) == U
        assert f(None, *good, *dims, *band, -1) == U
        assert f(None, *good, 70000, 4, 4, 8, 8, *band, 0) == N.ERR_TOO_LARGE
    # mode 4: feat, packed, initq, initq_x3, head, pix, taps, out
    f4 = lib.diinn_decode_initq_mode4_x3
    good = [one] * 8
    for i in range(8):
        assert f4(None, *[None if j == i else p for j, p in enumerate(good)], *dims, *band, 0) == E, i
    for i in (1, 2, 3, 4, 5):
        assert f4(None, *[odd if j == i else p for j, p in enumerate(good)], *dims, *band, 0) == E, i
    assert f4(None, *good, 1, 4, 4, 1, 8, 0, 1, 0) == E                                               # Hu < 2
    assert f4(None, *good, 1, 4, 4, 8, 1, *band, 0) == E                                              # Wu < 2
    assert f4(None, *good, *dims, 3, 3, 0) == E
    assert f4(None, *good, *dims, 0, 9, 0) == E
    assert f4(None, *good, *dims, *band, 7) == U


def test_kernel_resources_and_that_nothing_earlier_left(tmp_path):
    """The eleven code objects this path adds, by mangled name: ``pixel_chain_x3_kernel<false / true>``, the 512-row planes form
    ``initq_planes_x3_kernel<8..10>``, ``decode_bf16x3_kernel<20..22>`` (SIN | X3_INITQ | X3_QONLY) and ``<36..38>`` (SIN | X3_INITQ |
    X3_TAPS).  No scratch, no spilled vector register; the chain and the decode forms at the ONE wave per SIMD they are designed for
    (128 KiB park slab), the planes form at the two waves per SIMD of ``initq_planes_x3_kernel`` (one workgroup of eight waves per
    CU).  Every earlier instantiation of the two templates is still there under its name."""
    import diinn_amd._native as N
    import test_kernel_resources as R
    if not os.path.exists(R.READELF):
        pytest.skip("llvm-readelf (ROCm) not installed")
    ks = {k[".name"]: k for k in R.kernel_metadata(N.LIB_PATH, tmp_path)}
    park = 128 * 1024
    want = {"_Z21pixel_chain_x3_kernelILb0EEv16PixChainX3Params": (park, 1), "_Z21pixel_chain_x3_kernelILb1EEv16PixChainX3Params": (park, 1)}
    for s in range(3):
        want[f"_Z22initq_planes_x3_kernelILi{8 + s}EEv13InitqX3Params"] = (144 * 1024 + 10 * 1024, 2)
        want[f"_Z20decode_bf16x3_kernelILi{20 + s}EEv12DecodeParams"] = (park + 6 * 1024 + 16, 1)
        want[f"_Z20decode_bf16x3_kernelILi{36 + s}EEv12DecodeParams"] = (park + 30 * 1024 + 16, 1)
    listed = sorted(n for n in ks if R.base_name(n) in ("decode_bf16x3_kernel", "initq_planes_x3_kernel", "pixel_chain_x3_kernel"))
    for name, (lds, occ) in want.items():
        assert name in ks, (name, listed)
        k = ks[name]
        assert int(k[".private_segment_fixed_size"]) == 0 and not k.get(".uses_dynamic_stack"), name
        assert int(k[".vgpr_spill_count"]) == 0, name
        assert int(k[".group_segment_fixed_size"]) == lds, (name, k[".group_segment_fixed_size"])
        assert R.occupancy(k) == occ, (name, R.occupancy(k))
    assert sum(R.base_name(n) == "pixel_chain_x3_kernel" for n in ks) == 2
    for arg in (0, 1, 2, 4, 5, 6, 8, 9, 10, 12, 13, 14, 16, 17, 18, 32, 33, 34):
        assert f"_Z20decode_bf16x3_kernelILi{arg}EEv12DecodeParams" in ks, (arg, listed)
    for arg in (0, 1, 2, 4, 5, 6):
        assert f"_Z22initq_planes_x3_kernelILi{arg}EEv13InitqX3Params" in ks, (arg, listed)
    for name in ("_Z18pixel_chain_kernelILb0EEv14PixChainParams", "_Z18pixel_chain_kernelILb1EEv14PixChainParams"):
        assert name in ks, name


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("sin_mode", [0, 1, 2])
@pytest.mark.parametrize("mode", MODES)
def test_reference_fixtures(gold, dev, mode, sin_mode):
    """All seven cases of the mode: kernel against ref32 and against the emulation sheet within the contract; for the accurate
    sine ``max|hip - ref64| <= 3.0 x N'`` as well (the hardware sines: printed).

    Measured on an MI355X (worst case over the sine modes): max|hip - ref32| 3.8e-6 / 4.0e-6 / 3.4e-6 on the gain-2 case of modes 1 /
    2 / 4 and <= 1.1e-7 on every gain-1 case, against the contract's 1e-4; max|hip - emulation| <= 3.2e-6; max|hip - ref64| / N' at
    most 1.31 (modes 1 and 4, siren_9x14_36x56), 1.23 on a gain-2 case.  On the CPU a dropped product sits at >= 7 x N'."""
    noise = _noise(gold, mode)
    bad = []
    for name in NAMES:
        b, h, w, hu, wu, gain, fgain = _case(gold, mode, name)
        images = _images(_state_dict(mode, gain, fgain), mode, dev)
        feat = torch.from_numpy(synth.encoder_features(123, b, h, w)).to(dev)
        got = _decode_x3(feat, images, (hu, wu), mode, sin_mode=sin_mode)
        torch.cuda.synchronize()
        got = got.cpu().numpy()
        ref32, ref64 = _refs(gold, mode, name)
        em = _emulation(gold, mode, name)
        assert got.shape == ref32.shape
        err32, errem, e64 = (float(np.abs(got - r).max()) for r in (ref32, em, ref64))
        print(f"mode {mode} sin_mode {sin_mode} {name}: max|hip - ref32| = {err32:.3e}  max|hip - emulation| = {errem:.3e} "
              f"(contract {_tol(ref32):.1e}); max|hip - ref64| = {e64:.3e} = {e64 / noise[gain]:.2f} N' (N' = {noise[gain]:.3e})")
        if not err32 <= _tol(ref32):
            bad.append(f"{name}: ref32 {err32:.3e} > {_tol(ref32):.1e}")
        if not errem <= _tol(ref32):
            bad.append(f"{name}: emulation {errem:.3e} > {_tol(ref32):.1e}")
        if sin_mode == 0 and not e64 <= FACTOR * noise[gain]:
            bad.append(f"{name}: ref64 {e64:.3e} > {FACTOR} x {noise[gain]:.3e}")
    assert not bad, bad


@gpu
@pytest.mark.parametrize("name", ["b3_7x5_23x18", "small4x3_110x9"])
@pytest.mark.parametrize("mode", MODES)
def test_module_forward_is_the_functional_entry_and_chunks_change_no_bit(gold, dev, mode, name):
    """``ImplicitDecoder.forward`` with the three settings equals ``decode_features_initq(compute="bf16x3")`` bit for bit, under
    no_grad and with ``bsize``; in chunks of eight rows of planes (mode 4: six output rows and one tap row each way) it has the
    bits of one chunk.  It is not the fp32 path's result, and within the contract of it."""
    import diinn_amd.decoder as D
    b, h, w, hu, wu, gain, fgain = _case(gold, mode, name)
    sd = _state_dict(mode, gain, fgain)
    dec = _module(mode, sd, dev)
    feat = torch.from_numpy(synth.encoder_features(123, b, h, w)).to(dev)
    want = _decode_x3(feat, _images(sd, mode, dev), (hu, wu), mode)
    assert D.initq_chunk_rows(b, wu, dec.INITQ_CHUNK_BYTES) >= hu            # one chunk
    with torch.no_grad():
        whole = dec(feat, (hu, wu)).clone()
    assert torch.equal(whole, want)
    dec.INITQ_CHUNK_BYTES = 1                                                # on the instance
    assert D.initq_chunk_rows(b, wu, dec.INITQ_CHUNK_BYTES) == 8 < hu
    dec._pix_workspaces.clear()
    dec._tap_workspaces.clear()
    chunked = dec(feat, [hu, wu], 30000)
    assert next(iter(dec._pix_workspaces.values())).numel() == b * 8 * wu * 1280
    if mode == 4:
        assert next(iter(dec._tap_workspaces.values())).numel() == b * 8 * wu * 28
    assert torch.equal(whole, chunked)
    with pytest.raises(NotImplementedError):
        dec(feat, (hu, wu))                                                  # autograd
    dec.compute = "f32"
    with torch.no_grad():
        f32 = dec(feat, (hu, wu))
    assert not torch.equal(f32, whole)
    assert float((f32 - whole).abs().max()) <= TOL * max(1.0, float(f32.abs().max()))
    dec.compute, dec.hip_initq_modes_split_bf16 = "bf16x3", False
    with torch.no_grad(), pytest.raises(ValueError, match="fp32 only"):
        dec(feat, (hu, wu))


@gpu
@pytest.mark.parametrize("mode", MODES)
def test_row_bands_are_bit_equal_and_write_nothing_else(gold, dev, mode):
    """Bands that start at a chunk edge and beside one (mode 4 reads one more row each way, reflected at the IMAGE's edges only),
    and one band off multiples of 8 at both ends; a caller's ``pix`` of exactly the band's size."""
    b, h, w, hu, wu, gain, fgain = _case(gold, mode, "b3_7x5_23x18")
    images = _images(_state_dict(mode, gain, fgain), mode, dev)
    feat = torch.from_numpy(synth.encoder_features(123, b, h, w)).to(dev)
    full = _decode_x3(feat, images, (hu, wu), mode)
    ref32, _ = _refs(gold, mode, "b3_7x5_23x18")
    assert float(np.abs(full.cpu().numpy() - ref32).max()) <= _tol(ref32)
    for y0, y1 in ((0, 8), (1, 9), (8, 16), (hu - 1, hu), (0, 1), (3, 13), (16, hu)):
        out = torch.full((b, 3, hu, wu), CANARY, device=dev)
        got = _decode_x3(feat, images, (hu, wu), mode, rows=(y0, y1), out=out)
        assert got is out
        assert torch.equal(out[:, :, y0:y1], full[:, :, y0:y1]), (y0, y1)
        keep = torch.ones(hu, dtype=torch.bool, device=dev)
        keep[y0:y1] = False
        assert bool((out[:, :, keep] == CANARY).all()), (y0, y1)
    rows = 12 if mode == 4 else 10
    pix = torch.empty(b * rows * wu * 1280, device=dev)
    out = _decode_x3(feat, images, (hu, wu), mode, rows=(3, 13), pix=pix)
    assert torch.equal(out[:, :, 3:13], full[:, :, 3:13])
    with pytest.raises(ValueError, match="pix"):
        _decode_x3(feat, images, (hu, wu), mode, rows=(3, 14), pix=pix)


@gpu
@pytest.mark.parametrize("sin_mode", [0, 2])
def test_mode1_planes_forms_agree_bit_for_bit_and_the_512_row_form_leaves_the_slots_alone(gold, dev, sin_mode):
    """Mode 1 through the 512-row planes form against the 1280-row form on the same (zero-widened) image: the same output bits.  The
    512-row planes kernel on a poisoned buffer: channels 0..255 and 1024..1279 have the bits of the 1280-row kernel's, channels
    256..1023 still hold the poison."""
    import diinn_amd._native as N
    lib = N.load()
    b, h, w, hu, wu, gain, fgain = _case(gold, 1, GAIN2)
    images = _images(_state_dict(1, gain, fgain), 1, dev)
    packed, image, image_x3, _ = images
    feat = torch.from_numpy(synth.encoder_features(123, b, h, w)).to(dev)
    a = _decode_x3(feat, images, (hu, wu), 1, sin_mode=sin_mode)
    ref32, _ = _refs(gold, 1, GAIN2)
    assert float(np.abs(a.cpu().numpy() - ref32).max()) <= _tol(ref32)
    assert torch.equal(a, _decode_x3(feat, images, (hu, wu), 1, sin_mode=sin_mode, planes_rows=1280))
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    y0, y1 = 3, 22                                                           # ragged at both ends of the 8-row tiles
    geometry = (b, h, w, hu, wu, y0, y1, sin_mode)
    p512 = torch.full((b, y1 - y0, wu, 1280), CANARY, device=dev)
    p1280 = torch.full((b, y1 - y0, wu, 1280), CANARY, device=dev)
    N.check(lib.diinn_initq_planes_m1_x3(stream, _ptr(feat), _ptr(packed), _ptr(image), _ptr(image_x3), _ptr(p512), *geometry), "m1")
    N.check(lib.diinn_initq_planes_x3(stream, _ptr(feat), _ptr(packed), _ptr(image), _ptr(image_x3), _ptr(p1280), *geometry), "full")
    torch.cuda.synchronize()
    assert bool((p512[..., 256:1024] == CANARY).all())
    assert not bool((p1280 == CANARY).any())
    assert torch.equal(p512[..., :256].view(torch.int32), p1280[..., :256].view(torch.int32))
    assert torch.equal(p512[..., 1024:].view(torch.int32), p1280[..., 1024:].view(torch.int32))


@gpu
def test_mode4_with_a_centre_tap_head_is_mode3_split_with_that_tap_as_its_head(gold, dev):
    """Bit for bit, as in fp32: the layers are the same code, the centre tap's 256-term dot product runs in the 1x1 head's order, the
    eight zero taps add +0 and ``bias + t`` is ``t + bias``.  Separates the tap form on pixel records from the gather."""
    import diinn_amd.decoder as D
    b, h, w, hu, wu, gain, fgain = _case(gold, 4, "b3_7x5_23x18")
    sd4 = dict(_state_dict(4, gain, fgain))
    lw = np.zeros_like(sd4["last_layer.weight"])
    lw[:, :, 1, 1] = sd4["last_layer.weight"][:, :, 1, 1]
    sd4["last_layer.weight"] = lw
    sd3 = dict(sd4)
    sd3["last_layer.weight"] = np.ascontiguousarray(lw[:, :, 1:2, 1:2])
    feat = torch.from_numpy(synth.encoder_features(123, b, h, w)).to(dev)
    images = _images(sd4, 4, dev)
    got4 = _decode_x3(feat, images, (hu, wu), 4)
    packed3 = D.pack_state_dict(D.initq_body_state_dict(sd3), mode=3).to(dev)
    got3 = D.decode_features(feat, packed3, (hu, wu), initq=images[1], compute="bf16x3", initq_x3=images[2])
    assert float(got3.abs().max()) > 1e-3
    assert torch.equal(got4, got3)


@gpu
@pytest.mark.parametrize("mode", MODES)
def test_whole_model(dev, mode):
    """``DIINN(mode, init_q=True)`` with the switches against the same model in fp32: within the contract, and not the same bits."""
    import diinn_amd.modules as M
    torch.manual_seed(5)
    net = M.DIINN(mode=mode, init_q=True).to(dev).eval()
    net.decoder.hip_initq_modes = True
    x = torch.rand(1, 3, 12, 12, device=dev)
    with torch.no_grad():
        f32 = net(x, (24, 24), 30000)
        net.decoder.compute = "bf16x3"
        with pytest.raises(ValueError, match="fp32 only"):
            net(x, (24, 24), 30000)
        net.decoder.hip_initq_modes_split_bf16 = True
        got = net(x, (24, 24), 30000)
    assert tuple(got.shape) == (1, 3, 24, 24) and not torch.equal(got, f32)
    err = float((got - f32).abs().max())
    print(f"mode {mode}: whole model, split bf16 vs fp32 {err:.3e}")
    assert err <= TOL * max(1.0, float(f32.abs().max())), err
