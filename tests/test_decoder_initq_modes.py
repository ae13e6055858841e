"""Decoder ``init_q=True`` with modes 1, 2 and 4 on the HIP path (opt-in: ``ImplicitDecoder.hip_initq_modes``) -- the per-pixel
modulation chain ``pixel_chain_kernel`` with ``decode_kernel<SIN | DECODE_INITQ, KPART=false>`` (modes 1/2), the 512-row planes form
``initq_planes_kernel<SIN | INITQ_ROWS512>`` (mode 1) and the tap form ``decode_kernel<SIN | DECODE_INITQ | DECODE_TAPS>`` with
``head3x3_reflect_kernel`` (mode 4) -- against fixtures from the real reference (tests/golden/make_golden_initq_modes.py: fp32
output and its distance to the reference's own float64 run).

The contract is SURVEY section 8 d4, ``max|hip - ref32| <= 1e-4 * max(1, max|ref|)``, for every sine mode.  The accurate sine is
held to the noise-floor bound as well: ``max|hip - ref64| <= FACTOR * N`` with N the largest ``max|ref32 - ref64|`` over the
fixture cases of the same mode and gain (as tests/test_decoder_initq.py groups them) and FACTOR = 3.0 as in
tests/test_decoder_modes.py.  For the hardware sines the ratio is printed, not asserted, as there."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import diinn_amd.synth as synth
from conftest import ROOT

TOL = 1e-4
FACTOR = 3.0                      # tests/test_decoder_modes.py, tests/test_decoder_initq.py
MODES = (1, 2, 4)
NAMES = ["c1x1_2x2", "row1x9_2x30", "b3_7x5_23x18", "b2_12x10_31x27_gain2", "down16x12_8x6", "small4x3_110x9", "siren_9x14_36x56"]


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "diinn_golden_initq_modes.npz"))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
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


def _noise(g, mode):
    """N per gain: the largest max|ref32 - ref64| over the cases of that mode and gain."""
    n = {}
    for name in NAMES:
        gain = _case(g, mode, name)[5]
        n[gain] = max(n.get(gain, 0.0), float(np.abs(g[f"d64/{mode}/{name}"]).max()))
    return n


def _tol(ref):
    return TOL * max(1.0, float(np.abs(ref).max()))


def _module(mode, sd, dev=None, **kw):
    import diinn_amd.decoder as D
    dec = D.ImplicitDecoder(mode=mode, init_q=True, hip_initq_modes=True, **kw)
    dec.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    return (dec.to(dev) if dev is not None else dec).eval()


def _images(D, sd, mode, dev):
    packed = D.pack_state_dict(D.initq_body_state_dict(sd), mode=mode).to(dev)
    head = D.pack_head3x3(sd).to(dev) if mode == 4 else None
    return packed, D.pack_initq(sd).to(dev), head


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------
def test_fixture_file_holds_seven_cases_per_mode_within_a_third_of_the_contract(gold):
    assert len(gold.files) == 3 * len(MODES) * len(NAMES)
    for mode in MODES:
        for name in NAMES:
            b, h, w, hu, wu, gain, fgain = _case(gold, mode, name)
            ref32, _ = _refs(gold, mode, name)
            assert ref32.shape == (b, 3, hu, wu) and ref32.dtype == np.float32 and np.isfinite(ref32).all()
            d = float(np.abs(gold[f"d64/{mode}/{name}"]).max())
            assert 0.0 < d <= _tol(ref32) / 3.0, (mode, name, d)


def test_with_the_switch_off_every_call_refuses_as_before():
    import diinn_amd.decoder as D
    assert D.ImplicitDecoder.hip_initq_modes is False
    x = torch.zeros(1, 64, 4, 4)                      # CPU tensors: a refusal that looked at the device would raise RuntimeError
    for mode in MODES:
        for kw in ({}, {"hip_initq_modes": False}):
            dec = D.ImplicitDecoder(mode=mode, init_q=True, **kw)
            assert dec.hip_initq_modes is False
            for ctx in (torch.no_grad(), torch.enable_grad()):
                with ctx, pytest.raises(NotImplementedError, match="mode 3"):
                    dec(x, (8, 8))
            with torch.no_grad(), pytest.raises(NotImplementedError, match="mode 3"):
                dec(x, (8, 8), 30000)
    img = torch.zeros(4)
    for mode in MODES:                                # the old functional entry refuses whatever the switch says
        with pytest.raises(NotImplementedError, match="mode 3"):
            D.decode_features(x, img, (8, 8), mode=mode, initq=img)


def test_with_the_switch_on_only_the_device_is_missing():
    """Fails on the parent commit: there the constructor has no such keyword and the call raises NotImplementedError."""
    import diinn_amd.decoder as D
    import diinn_amd.modules as M
    x = torch.zeros(1, 64, 4, 4)
    for mode in MODES:
        dec = D.ImplicitDecoder(mode=mode, init_q=True, hip_initq_modes=True)
        for bsize in (None, 30000):
            with torch.no_grad(), pytest.raises(RuntimeError, match="ROCm GPU"):
                dec(x, (8, 8), bsize)
        net = M.DIINN(mode=mode, init_q=True)
        net.decoder.hip_initq_modes = True            # the one line a user writes
        with torch.no_grad(), pytest.raises(RuntimeError, match="ROCm GPU"):
            net.decoder(x, (8, 8), 30000)
        img = torch.zeros(4)
        with pytest.raises(RuntimeError, match="ROCm GPU"):
            D.decode_features_initq(x, img, img, (8, 8), mode, head=img)
    # mode 3 and init_q=False are untouched by the switch
    with torch.no_grad(), pytest.raises(RuntimeError, match="ROCm GPU"):
        D.ImplicitDecoder(mode=3, init_q=True, hip_initq_modes=True)(x, (8, 8), 30000)
    with pytest.raises(NotImplementedError, match="autograd"):
        D.ImplicitDecoder(mode=3, init_q=True, hip_initq_modes=True)(x, (8, 8))


def test_out_of_scope_calls_keep_raising_with_the_switch_on():
    import diinn_amd.decoder as D
    import diinn_amd.modules as M
    x = torch.zeros(1, 64, 4, 4)
    img = torch.zeros(4)
    for mode in MODES:
        # autograd, also with the training switches of the other paths
        for kw in ({}, {"hip_autograd": True}, {"hip_autograd_mode4": True}, {"hip_autograd": True, "hip_autograd_mode4": True}):
            dec = D.ImplicitDecoder(mode=mode, init_q=True, hip_initq_modes=True, **kw)
            with pytest.raises(NotImplementedError, match="inference only"):
                dec(x, (8, 8))
            with pytest.raises(NotImplementedError, match="inference only"):
                dec.requires_grad_(False)(x.clone().requires_grad_(True), (8, 8))
        # the bf16 arithmetics
        for compute in ("bf16", "bf16_full", "bf16x3"):
            with torch.no_grad(), pytest.raises(ValueError, match="fp32"):
                D.ImplicitDecoder(mode=mode, init_q=True, hip_initq_modes=True, compute=compute)(x, (8, 8))
        # graph replay
        with pytest.raises(NotImplementedError, match="graphs"):
            M.DIINN(mode=mode, init_q=True, graphs=True)
        # the sharded forward
        net = M.DIINN(mode=mode, init_q=True)
        net.decoder.hip_initq_modes = True
        with pytest.raises(NotImplementedError, match="mode 4" if mode == 4 else "init_q"):
            net.forward_sharded(torch.zeros(1, 3, 4, 4), (8, 8))
    # the new functional entry is for modes 1, 2, 4; the planes form is mode 1's choice alone
    with pytest.raises(NotImplementedError, match="modes 1, 2 and 4"):
        D.decode_features_initq(x, img, img, (8, 8), 3)
    with pytest.raises(ValueError, match="planes_rows"):
        D.decode_features_initq(x, img, img, (8, 8), 2, planes_rows=512)
    # windows and tiles have no init_q form
    with pytest.raises(TypeError):
        D.decode_window(x, 0, 4, img, (8, 8), (0, 8), initq=img)
    with pytest.raises(TypeError):
        D.decode_tile(img, 0, (1, 4, 4), img, (8, 8), (0, 8), (0, 8), torch.zeros(1, 3, 8, 8), initq=img)


def test_restatement_matches_the_reference_in_fp32_and_float64(gold):
    """``initq_modes_forward_reference`` against the real reference: fp32 within the contract, float64 within 1e-6 of the
    reference's float64 (the bound tests/test_decoder_initq.py uses for its restatement; measured here: 1e-17 .. 1e-14)."""
    import diinn_amd.decoder as D
    for mode in MODES:
        for name in NAMES:
            b, h, w, hu, wu, gain, fgain = _case(gold, mode, name)
            sd = _state_dict(mode, gain, fgain)
            feat = torch.from_numpy(synth.encoder_features(123, b, h, w))
            ref32, ref64 = _refs(gold, mode, name)
            r32 = D.initq_modes_forward_reference(sd, feat, (hu, wu), mode, torch.float32)
            assert r32.dtype == torch.float32 and tuple(r32.shape) == ref32.shape
            r64 = D.initq_modes_forward_reference(sd, feat, (hu, wu), mode)
            assert r64.dtype == torch.float64
            e32, e64 = float(np.abs(r32.numpy() - ref32).max()), float(np.abs(r64.numpy() - ref64).max())
            print(f"mode {mode} {name}: fp32 restatement vs ref32 {e32:.2e}, float64 restatement vs ref64 {e64:.2e}")
            assert e32 <= _tol(ref32), (mode, name)
            assert e64 <= 1e-6, (mode, name)
    with pytest.raises(ValueError, match="modes 1, 2 and 4"):
        D.initq_modes_forward_reference({}, torch.zeros(1, 64, 2, 2), (4, 4), 3)


def test_new_entry_points_validate_before_they_touch_a_device():
    import diinn_amd._native as N
    lib = N.load()
    one, odd = C.c_void_p(16), C.c_void_p(8)
    dims, band = (1, 4, 4, 8, 8), (0, 8)
    assert lib.diinn_abi_version() == 11
    # byte counts: the tap rows of mode 4, one more row each way, clipped to the image
    assert lib.diinn_initq_mode4_pix_bytes(2, 20, 10, 0, 8) == 2 * 9 * 10 * 5120
    assert lib.diinn_initq_mode4_pix_bytes(2, 20, 10, 8, 16) == 2 * 10 * 10 * 5120
    assert lib.diinn_initq_mode4_pix_bytes(1, 20, 10, 19, 20) == 2 * 10 * 5120
    assert lib.diinn_initq_mode4_pix_bytes(1, 20, 10, 0, 20) == lib.diinn_initq_pix_bytes(1, 10, 20)
    for bad in ((0, 20, 10, 0, 8), (1, 1, 10, 0, 1), (1, 20, 1, 0, 8), (1, 20, 10, 8, 8), (1, 20, 10, 0, 21), (1, 20, 10, -1, 4)):
        assert lib.diinn_initq_mode4_pix_bytes(*bad) == 0, bad
    # the 512-row planes form
    assert lib.diinn_initq_planes_m1(None, None, one, one, one, *dims, *band, 0) == N.ERR_INVALID_ARG
    assert lib.diinn_initq_planes_m1(None, one, one, one, None, *dims, *band, 0) == N.ERR_INVALID_ARG
    assert lib.diinn_initq_planes_m1(None, one, one, one, one, *dims, 4, 4, 0) == N.ERR_INVALID_ARG
    assert lib.diinn_initq_planes_m1(None, one, one, one, one, *dims, 0, 9, 0) == N.ERR_INVALID_ARG
    assert lib.diinn_initq_planes_m1(None, one, one, one, one, *dims, *band, 7) == N.ERR_UNSUPPORTED
    # the pixel chain
    assert lib.diinn_pixel_chain(None, None, one, 1, 8, 8, 0) == N.ERR_INVALID_ARG
    assert lib.diinn_pixel_chain(None, one, None, 1, 8, 8, 1) == N.ERR_INVALID_ARG
    assert lib.diinn_pixel_chain(None, odd, one, 1, 8, 8, 0) == N.ERR_INVALID_ARG             # 16-byte seeds
    for b, wu, rows in ((0, 8, 8), (1, 0, 8), (1, 8, 0), (1, 8, -3)):
        assert lib.diinn_pixel_chain(None, one, one, b, wu, rows, 1) == N.ERR_INVALID_ARG
    assert lib.diinn_pixel_chain(None, one, one, 70000, 8, 8, 0) == N.ERR_TOO_LARGE
    assert lib.diinn_pixel_chain(None, one, one, 1, 8, 8 * 65536, 0) == N.ERR_TOO_LARGE
    # the band decodes
    assert lib.diinn_decode_initq_qonly_band(None, one, one, None, *dims, *band, 0) == N.ERR_INVALID_ARG
    assert lib.diinn_decode_initq_qonly_band(None, one, one, one, 0, 4, 4, 8, 8, *band, 0) == N.ERR_INVALID_ARG
    assert lib.diinn_decode_initq_qonly_band(None, one, one, one, *dims, 3, 3, 0) == N.ERR_INVALID_ARG
    assert lib.diinn_decode_initq_qonly_band(None, one, one, one, *dims, *band, 7) == N.ERR_UNSUPPORTED
    assert lib.diinn_decode_initq_mode4_band(None, one, one, None, one, one, *dims, *band, 0) == N.ERR_INVALID_ARG
    assert lib.diinn_decode_initq_mode4_band(None, one, one, one, None, one, *dims, *band, 0) == N.ERR_INVALID_ARG
    assert lib.diinn_decode_initq_mode4_band(None, one, one, one, one, one, 1, 4, 4, 8, 1, *band, 0) == N.ERR_INVALID_ARG   # Wu < 2
    assert lib.diinn_decode_initq_mode4_band(None, one, one, one, one, one, *dims, 0, 9, 0) == N.ERR_INVALID_ARG
    assert lib.diinn_decode_initq_mode4_band(None, one, one, one, one, one, *dims, *band, 7) == N.ERR_UNSUPPORTED
    # all in order: a bad argument of a LATER launch is refused before the first one
    for fn in (lib.diinn_decode_initq_mode1, lib.diinn_decode_initq_mode2):
        assert fn(None, one, one, one, one, None, *dims, *band, 0) == N.ERR_INVALID_ARG
        assert fn(None, None, one, one, one, one, *dims, *band, 0) == N.ERR_INVALID_ARG
        assert fn(None, one, one, one, odd, one, *dims, *band, 0) == N.ERR_INVALID_ARG
        assert fn(None, one, one, one, one, one, *dims, 8, 8, 0) == N.ERR_INVALID_ARG
        assert fn(None, one, one, one, one, one, *dims, *band, 3) == N.ERR_UNSUPPORTED
    f4 = lib.diinn_decode_initq_mode4
    assert f4(None, one, one, one, None, one, one, one, *dims, *band, 0) == N.ERR_INVALID_ARG
    assert f4(None, one, one, one, one, one, None, one, *dims, *band, 0) == N.ERR_INVALID_ARG
    assert f4(None, one, one, one, one, one, one, None, *dims, *band, 0) == N.ERR_INVALID_ARG
    assert f4(None, one, one, one, one, one, one, one, 1, 4, 4, 1, 8, 0, 1, 0) == N.ERR_INVALID_ARG                        # Hu < 2
    assert f4(None, one, one, one, one, one, one, one, *dims, *band, -1) == N.ERR_UNSUPPORTED


def test_new_kernel_instantiations_use_no_scratch(tmp_path):
    """The eleven code objects this path adds to the shipped library, picked out by name: no scratch, no spilled register, one wave
    per SIMD; the tap form of init_q keeps the 27 KiB head table next to the (unused) Q0 rows in LDS like mode 4's."""
    import diinn_amd._native as N
    import test_kernel_resources as R
    if not os.path.exists(R.READELF):
        pytest.skip("llvm-readelf (ROCm) not installed")
    ks = {k[".name"]: k for k in R.kernel_metadata(N.LIB_PATH, tmp_path)}
    want = [f"_Z13decode_kernelILi{4 + s}ELb0ELb0ELb0EEv12DecodeParams" for s in range(3)]            # modes 1/2: SIN | DECODE_INITQ, KPART = false
    taps = [f"_Z13decode_kernelILi{12 + s}ELb1ELb0ELb0EEv12DecodeParams" for s in range(3)]           # mode 4: SIN | DECODE_INITQ | DECODE_TAPS
    want += taps
    want += [f"_Z19initq_planes_kernelILi{8 + s}EEv11InitqParams" for s in range(3)]                  # mode 1: SIN | INITQ_ROWS512
    want += ["_Z18pixel_chain_kernelILb0EEv14PixChainParams", "_Z18pixel_chain_kernelILb1EEv14PixChainParams"]
    for name in want:
        assert name in ks, (name, sorted(n for n in ks if "decode_kernel" in n or "chain" in n or "initq_planes" in n))
        k = ks[name]
        assert int(k[".private_segment_fixed_size"]) == 0 and not k.get(".uses_dynamic_stack"), name
        assert int(k[".vgpr_spill_count"]) == 0 and int(k[".sgpr_spill_count"]) == 0, name
        assert R.occupancy(k) >= 1, name
    for name in taps:
        assert int(ks[name][".group_segment_fixed_size"]) == (3 + 27) * 256 * 4 + 16
    assert sum(R.base_name(n) == "pixel_chain_kernel" for n in ks) == 2


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("sin_mode", [0, 1, 2])
@pytest.mark.parametrize("mode", MODES)
def test_reference_fixtures(gold, dev, mode, sin_mode):
    noise = _noise(gold, mode)
    bad = []
    for name in NAMES:
        b, h, w, hu, wu, gain, fgain = _case(gold, mode, name)
        dec = _module(mode, _state_dict(mode, gain, fgain), dev, sin_mode=sin_mode)
        feat = torch.from_numpy(synth.encoder_features(123, b, h, w)).to(dev)
        with torch.no_grad():
            got = dec(feat, (hu, wu)).cpu().numpy()
        ref32, ref64 = _refs(gold, mode, name)
        err = float(np.abs(got - ref32).max())
        e64 = float(np.abs(got - ref64).max())
        print(f"mode {mode} sin_mode {sin_mode} {name}: max|hip - ref32| = {err:.3e} (contract {_tol(ref32):.1e}); "
              f"max|hip - ref64| = {e64:.3e} = {e64 / noise[gain]:.2f} N (N = {noise[gain]:.3e})")
        if not err <= _tol(ref32):
            bad.append(f"{name}: {err:.3e} > {_tol(ref32):.1e}")
        if sin_mode == 0 and not e64 <= FACTOR * noise[gain]:
            bad.append(f"{name}: {e64:.3e} > {FACTOR} x {noise[gain]:.3e}")
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["b3_7x5_23x18", "small4x3_110x9"])
@pytest.mark.parametrize("mode", MODES)
def test_chunks_of_eight_rows_change_no_bit(gold, dev, mode, name):
    import diinn_amd.decoder as D
    b, h, w, hu, wu, gain, fgain = _case(gold, mode, name)
    dec = _module(mode, _state_dict(mode, gain, fgain), dev)
    feat = torch.from_numpy(synth.encoder_features(123, b, h, w)).to(dev)
    assert D.initq_chunk_rows(b, wu, dec.INITQ_CHUNK_BYTES) >= hu            # one chunk
    with torch.no_grad():
        whole = dec(feat, (hu, wu)).clone()
    dec.INITQ_CHUNK_BYTES = 1                                                # on the instance
    assert D.initq_chunk_rows(b, wu, dec.INITQ_CHUNK_BYTES) == 8 < hu
    dec._pix_workspaces.clear()
    dec._tap_workspaces.clear()
    with torch.no_grad():
        chunked = dec(feat, (hu, wu), 30000)
    # eight rows of planes per chunk; for mode 4 they are the TAP rows (six output rows + one each way), as are the taps
    assert next(iter(dec._pix_workspaces.values())).numel() == b * 8 * wu * 1280
    if mode == 4:
        assert next(iter(dec._tap_workspaces.values())).numel() == b * 8 * wu * 28
    assert torch.equal(whole, chunked)
    ref32, _ = _refs(gold, mode, name)
    assert float(np.abs(whole.cpu().numpy() - ref32).max()) <= _tol(ref32)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_row_bands_are_bit_equal_and_write_nothing_else(gold, dev, mode):
    """Bands that start at a chunk edge and beside one: y0 in {0, 1, 8, Hu - 1} (mode 4 reads one more row each way, reflected at
    the IMAGE's edges only), and one band off multiples of 8 at both ends."""
    import diinn_amd.decoder as D
    b, h, w, hu, wu, gain, fgain = _case(gold, mode, "b3_7x5_23x18")
    sd = _state_dict(mode, gain, fgain)
    packed, image, head = _images(D, sd, mode, dev)
    feat = torch.from_numpy(synth.encoder_features(123, b, h, w)).to(dev)
    full = D.decode_features_initq(feat, packed, image, (hu, wu), mode, head=head)
    ref32, _ = _refs(gold, mode, "b3_7x5_23x18")
    assert float(np.abs(full.cpu().numpy() - ref32).max()) <= _tol(ref32)
    for y0, y1 in ((0, 8), (1, 9), (8, 16), (hu - 1, hu), (0, 1), (3, 13), (16, hu)):
        out = torch.full((b, 3, hu, wu), -7.25, device=dev)
        got = D.decode_features_initq(feat, packed, image, (hu, wu), mode, head=head, rows=(y0, y1), out=out)
        assert got is out
        assert torch.equal(out[:, :, y0:y1], full[:, :, y0:y1]), (y0, y1)
        keep = torch.ones(hu, dtype=torch.bool, device=dev)
        keep[y0:y1] = False
        assert bool((out[:, :, keep] == -7.25).all()), (y0, y1)
    # a caller's workspace of exactly the band's size; a smaller one is refused
    rows = 12 if mode == 4 else 10
    pix = torch.empty(b * rows * wu * 1280, device=dev)
    out = D.decode_features_initq(feat, packed, image, (hu, wu), mode, head=head, rows=(3, 13), pix=pix)
    assert torch.equal(out[:, :, 3:13], full[:, :, 3:13])
    with pytest.raises(ValueError, match="pix"):
        D.decode_features_initq(feat, packed, image, (hu, wu), mode, head=head, rows=(3, 14), pix=pix)


@pytest.mark.gpu
def test_mode4_with_a_centre_tap_head_is_mode3_with_that_tap_as_its_head(gold, dev):
    """Bit for bit: the layers are the same code, the centre tap's 256-term dot product runs in the 1x1 head's order, the eight zero
    taps add +0 and ``bias + t`` is ``t + bias``.  Separates the tap form on pixel records from the gather."""
    import diinn_amd.decoder as D
    b, h, w, hu, wu, gain, fgain = _case(gold, 4, "b3_7x5_23x18")
    sd4 = dict(_state_dict(4, gain, fgain))
    lw = np.zeros_like(sd4["last_layer.weight"])
    lw[:, :, 1, 1] = sd4["last_layer.weight"][:, :, 1, 1]
    sd4["last_layer.weight"] = lw
    sd3 = dict(sd4)
    sd3["last_layer.weight"] = np.ascontiguousarray(lw[:, :, 1:2, 1:2])
    feat = torch.from_numpy(synth.encoder_features(123, b, h, w)).to(dev)
    packed4, image, head = _images(D, sd4, 4, dev)
    got4 = D.decode_features_initq(feat, packed4, image, (hu, wu), 4, head=head)
    packed3 = D.pack_state_dict(D.initq_body_state_dict(sd3), mode=3).to(dev)
    got3 = D.decode_features(feat, packed3, (hu, wu), initq=image)
    assert float(got3.abs().max()) > 1e-3
    assert torch.equal(got4, got3)


@pytest.mark.gpu
@pytest.mark.parametrize("sin_mode", [0, 2])
def test_mode1_planes_forms_and_mode2_with_zero_feature_columns_agree_bit_for_bit(gold, dev, sin_mode):
    """Mode 1 through the 512-row planes form against mode 1 forced through the 1280-row form, and mode 2 with ``K_i[:, 256:] = 0``
    against mode 1 with the same remaining tensors: BIT FOR BIT, because the accumulation order is the same.  Channels 0..255 and
    1024..1279 come from the same ``gemm_pair`` in the same k order whichever wave runs it; in the 1280-row form the seed of layer i
    is ``bK_i`` plus 576 products with a zero weight, which add +-0 to the accumulator and leave ``bK_i``; the chain and the layers
    are then the same instructions on the same numbers."""
    import diinn_amd.decoder as D
    b, h, w, hu, wu, gain, fgain = _case(gold, 1, "b2_12x10_31x27_gain2")
    sd1 = _state_dict(1, gain, fgain)
    feat = torch.from_numpy(synth.encoder_features(123, b, h, w)).to(dev)
    packed1, image, _ = _images(D, sd1, 1, dev)
    a = D.decode_features_initq(feat, packed1, image, (hu, wu), 1, sin_mode=sin_mode)
    ref32, _ = _refs(gold, 1, "b2_12x10_31x27_gain2")
    assert float(np.abs(a.cpu().numpy() - ref32).max()) <= _tol(ref32)
    wide = D.decode_features_initq(feat, packed1, image, (hu, wu), 1, sin_mode=sin_mode, planes_rows=1280)
    assert torch.equal(a, wide)
    sd2 = dict(sd1)
    for i in (1, 2, 3):
        k = np.zeros((256, 832, 1, 1), np.float32)
        k[:, :256] = sd1[f"K.{i}.0.weight"]
        sd2[f"K.{i}.0.weight"] = k
    packed2, image2, _ = _images(D, sd2, 2, dev)
    assert torch.equal(packed1, packed2) and torch.equal(image, image2)
    as2 = D.decode_features_initq(feat, packed2, image2, (hu, wu), 2, sin_mode=sin_mode)
    assert torch.equal(a, as2)
    # and the module of mode 2 on those tensors, through the chunked forward
    with torch.no_grad():
        assert torch.equal(_module(2, sd2, dev, sin_mode=sin_mode)(feat, (hu, wu)), a)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_whole_model(dev, mode):
    import diinn_amd.decoder as D
    import diinn_amd.modules as M
    torch.manual_seed(5)
    lit = M.SRLitModule(arch="diinn", mode=mode, init_q=True).to(dev).eval()
    x = torch.rand(1, 3, 12, 12, device=dev)
    with torch.no_grad(), pytest.raises(NotImplementedError, match="mode 3"):
        lit(x, (24, 24), 30000)
    lit.net.decoder.hip_initq_modes = True
    with torch.no_grad():
        got = lit(x, (24, 24), 30000)
        feat = lit.net.encoder(x)
        ref = D.initq_modes_forward_reference(dict(lit.net.decoder.state_dict()), feat, (24, 24), mode)
    assert tuple(got.shape) == (1, 3, 24, 24)
    err = float((got.double() - ref).abs().max())
    print(f"mode {mode}: whole model vs float64 restatement {err:.3e}")
    assert err <= TOL * max(1.0, float(ref.abs().max())), err
