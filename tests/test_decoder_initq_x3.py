"""Decoder ``init_q=True`` (mode 3) in split-bf16 arithmetic, behind ``ImplicitDecoder.hip_initq_split_bf16``:
``initq_planes_x3_kernel`` (both per-pixel GEMMs as three bf16 MFMA products, fp32 accumulation) and the init_q form of
``decode_bf16x3_kernel``, against the real-reference fixtures of tests/golden/diinn_golden_initq.npz.

The contract is the fp32 path's, ``max|hip - ref32| <= 1e-4 * max(1, max|ref|)``, for every sine mode.  The noise-floor ratio
``max|hip - ref64| / N`` is printed and asserted for no mode: the CPU emulation of this arithmetic already lies at ~10 N on the
gain-3 case.  The planes are held to ``4 x`` the error of the emulated split against a float64 product of the same fp32 operands,
separately for the Wx rows and the Q0 rows (the factor covers the MFMA's summation order against a matmul's; a dropped or
doubled term moves the error by ~300 x)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import diinn_amd.synth as synth
from conftest import ROOT

TOL = 1e-4
PLANES_FACTOR = 4.0
INV_2PI = np.float32(0.15915494309189533577)


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "diinn_golden_initq.npz"))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def _cases(g):
    out = []
    for k in g.files:
        if k.startswith("meta/"):
            b, h, w, hu, wu, gain, fgain = g[k]
            out.append((k[5:], int(b), int(h), int(w), int(hu), int(wu), float(gain), float(fgain)))
    return out


def _case(g, name):
    return next(c for c in _cases(g) if c[0] == name)


def _state_dict(gain=1.0, fgain=1.0, seed=123):
    sd = synth.decoder_state_dict(seed, gain, mode=3, init_q=True)
    sd["first_layer.0.weight"] = (sd["first_layer.0.weight"] * np.float32(fgain)).astype(np.float32)
    return sd


def _noise(g):
    """N per gain: the largest max|ref32 - ref64| over the cases of that gain."""
    n = {}
    for name, *_, gain, _f in _cases(g):
        n[gain] = max(n.get(gain, 0.0), float(np.abs(g[f"d64/{name}"]).max()))
    return n


def _tol(ref):
    return TOL * max(1.0, float(np.abs(ref).max()))


def _module(sd, dev=None, **kw):
    import diinn_amd.decoder as D
    kw.setdefault("hip_initq_split_bf16", True)
    kw.setdefault("compute", "bf16x3")
    dec = D.ImplicitDecoder(mode=3, init_q=True, **kw)
    dec.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return (dec.to(dev) if dev is not None else dec).eval()


def _images(sd, dev):
    import diinn_amd.decoder as D
    return (D.pack_state_dict(D.initq_body_state_dict(sd), mode=3).to(dev), D.pack_initq(sd).to(dev), D.pack_initq_x3(sd).to(dev))


def _bf16_rne(v):
    """fp32 array -> (bits of bf16(v) as uint16, bf16(v) as fp32): round to nearest even on the upper half."""
    u = np.ascontiguousarray(v, np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    return r, (r.astype(np.uint32) << 16).view(np.float32)


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------
def test_emulated_split_arithmetic_meets_the_contract_on_every_fixture(gold):
    import diinn_amd.decoder as D
    noise = _noise(gold)
    assert len(_cases(gold)) == 8
    for name, b, h, w, hu, wu, gain, fgain in _cases(gold):
        sd = _state_dict(gain, fgain)
        feat = torch.from_numpy(synth.encoder_features(123, b, h, w))
        ref32 = gold[f"out/{name}"]
        ref64 = ref32.astype(np.float64) + gold[f"d64/{name}"].astype(np.float64)
        emu = D.initq_forward_reference(sd, feat, (hu, wu), torch.float32, split_bf16=True)
        assert emu.dtype == torch.float32 and tuple(emu.shape) == ref32.shape
        err = float(np.abs(emu.numpy() - ref32).max())
        e64 = float(np.abs(emu.numpy() - ref64).max())
        print(f"{name}: max|emu - ref32| = {err:.3e} (contract {_tol(ref32):.2e}); max|emu - ref64| = {e64 / noise[gain]:.2f} N")
        assert err <= _tol(ref32), name
    with pytest.raises(ValueError, match="float32"):
        D.initq_forward_reference(sd, feat, (hu, wu), torch.float64, split_bf16=True)


def test_pack_initq_x3_places_every_value_where_the_layout_says():
    """From the layout comment (diinn_layout.h "the init_q SPLIT image"): [og 4][group 4][tap 9][M-tile 2][hi, lo][lane 64][j 8]
    bf16, then BQ0 [256], the validity word, three zero floats."""
    import diinn_amd._native as N
    import diinn_amd.decoder as D
    lib = N.load()
    n = lib.diinn_initq_x3_packed_floats()
    assert n == 4 * 4 * 9 * 2 * 2 * 256 + 256 + 4 == 147716
    rng = np.random.default_rng(11)
    q0w = rng.standard_normal((256, 576)).astype(np.float32)
    q0w[0, :4] = [0.0, -0.0, 1.0, 3.0e-39]                                           # zeros, an exact bf16, a subnormal
    q0b = (7000.0 + np.arange(256, dtype=np.float32))
    img = D.pack_initq_x3({"Q.0.0.weight": q0w.reshape(256, 576, 1, 1), "Q.0.0.bias": q0b}).numpy()
    assert img.shape == (n,) and img.dtype == np.float32
    nq = 4 * 4 * 9 * 2 * 2 * 256
    pieces = img[:nq].view(np.uint16).reshape(4, 4, 9, 2, 2, 64, 8)                  # [og][group][tap][mt][hi, lo][lane][j]
    og, g, tap, mt, lane, j = np.meshgrid(np.arange(4), np.arange(4), np.arange(9), np.arange(2), np.arange(64), np.arange(8),
                                          indexing="ij")
    o = 64 * og + 32 * mt + (lane & 31)
    c = 16 * g + 8 * (lane >> 5) + j
    v = (q0w * INV_2PI).astype(np.float32)[o, c * 9 + tap]                          # divided in fp32 BEFORE the split
    hi_bits, hi = _bf16_rne(v)
    lo_bits, lo = _bf16_rne(v - hi)
    assert np.array_equal(pieces[:, :, :, :, 0], hi_bits)
    assert np.array_equal(pieces[:, :, :, :, 1], lo_bits)
    assert float(np.abs((hi.astype(np.float64) + lo) - v).max()) <= 2.0 ** -16 * float(np.abs(v).max())
    # every Q0w element appears exactly once
    assert np.array_equal(np.sort((o * 576 + c * 9 + tap).ravel()), np.arange(256 * 576))
    assert np.array_equal(img[nq:nq + 256], q0b * INV_2PI)
    assert img[nq + 256:nq + 257].view(np.uint32)[0] == N.INITQ_X3_MAGIC == 0x44495833
    assert not img[nq + 257:].any()
    # the other images keep their sizes
    assert lib.diinn_initq_packed_floats() == 150020 and lib.diinn_packed_weight_floats() == 4691204
    # bad arguments: status 1, nothing written
    buf = np.zeros(n, np.float32)
    f = N.fptr
    assert lib.diinn_pack_initq_x3(None, f(q0b), f(buf)) == 1
    assert lib.diinn_pack_initq_x3(f(q0w), None, f(buf)) == 1
    assert lib.diinn_pack_initq_x3(f(q0w), f(q0b), None) == 1
    assert not buf.any()
    # the launch functions validate before they touch a device
    one = C.c_void_p(16)
    assert lib.diinn_initq_planes_x3(None, one, one, one, None, one, 1, 4, 4, 8, 8, 0, 8, 0) == 1
    assert lib.diinn_initq_planes_x3(None, None, one, one, one, one, 1, 4, 4, 8, 8, 0, 8, 0) == 1
    assert lib.diinn_initq_planes_x3(None, one, one, one, one, one, 1, 4, 4, 8, 8, 4, 4, 0) == 1
    assert lib.diinn_initq_planes_x3(None, one, one, one, one, one, 1, 4, 4, 8, 8, 0, 9, 0) == 1
    assert lib.diinn_initq_planes_x3(None, one, one, one, one, one, 1, 4, 4, 8, 8, 0, 8, 3) == 2      # no such sine mode
    assert lib.diinn_decode_initq_band_x3(None, one, one, None, 1, 4, 4, 8, 8, 0, 8, 0) == 1
    assert lib.diinn_decode_initq_band_x3(None, one, one, one, 0, 4, 4, 8, 8, 0, 8, 0) == 1
    assert lib.diinn_decode_initq_x3(None, one, one, one, one, one, None, 1, 4, 4, 8, 8, 0, 8, 0) == 1
    assert lib.diinn_decode_initq_x3(None, one, one, one, None, one, one, 1, 4, 4, 8, 8, 0, 8, 0) == 1
    assert lib.diinn_abi_version() == 11


def test_switch_and_refusals_touch_no_device():
    """Everything below is called with CPU tensors: a refusal that depended on the device would raise the "ROCm GPU" RuntimeError."""
    import diinn_amd.decoder as D
    import diinn_amd.modules as M
    x = torch.zeros(1, 64, 4, 4)
    assert D.ImplicitDecoder.hip_initq_split_bf16 is False and D.ImplicitDecoder(mode=3, init_q=True).hip_initq_split_bf16 is False
    # the switch on: only the device is missing (the fp32-only refusal is gone), as a keyword and as an attribute
    with torch.no_grad(), pytest.raises(RuntimeError, match="ROCm GPU"):
        D.ImplicitDecoder(mode=3, init_q=True, compute="bf16x3", hip_initq_split_bf16=True)(x, (8, 8))
    dec = D.ImplicitDecoder(mode=3, init_q=True, compute="bf16x3")
    dec.hip_initq_split_bf16 = True
    with torch.no_grad(), pytest.raises(RuntimeError, match="ROCm GPU"):
        dec(x, (8, 8))
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        dec(x, (8, 8), 30000)
    for compute in ("bf16", "bf16_full"):
        with torch.no_grad(), pytest.raises(ValueError, match="fp32"):
            D.ImplicitDecoder(mode=3, init_q=True, compute=compute, hip_initq_split_bf16=True)(x, (8, 8))
    # autograd stays closed, with and without hip_autograd
    for kw in ({}, {"hip_autograd": True}):
        with pytest.raises(NotImplementedError, match="autograd"):
            D.ImplicitDecoder(mode=3, init_q=True, compute="bf16x3", hip_initq_split_bf16=True, **kw)(x, (8, 8))
    # init_q with modes 1/2/4: as before, with and without hip_initq_modes
    for mode in (1, 2, 4):
        with torch.no_grad(), pytest.raises(NotImplementedError, match="mode 3"):
            D.ImplicitDecoder(mode=mode, init_q=True, compute="bf16x3", hip_initq_split_bf16=True)(x, (8, 8))
        with torch.no_grad(), pytest.raises(ValueError, match="fp32"):
            D.ImplicitDecoder(mode=mode, init_q=True, compute="bf16x3", hip_initq_split_bf16=True, hip_initq_modes=True)(x, (8, 8))
    with pytest.raises(NotImplementedError, match="graphs"):
        M.DIINN(mode=3, init_q=True, graphs=True)
    # the switch off: the present refusal
    with torch.no_grad(), pytest.raises(ValueError, match="fp32"):
        D.ImplicitDecoder(mode=3, init_q=True, compute="bf16x3")(x, (8, 8))
    # set_split_bf16 does what it did: it does not flip the switch
    net = M.DIINN(mode=3, init_q=True).set_split_bf16()
    assert net.decoder.compute == "bf16x3" and net.encoder.hip_split_bf16 and net.decoder.hip_initq_split_bf16 is False
    # the functional entry
    img = torch.zeros(4)
    with pytest.raises(ValueError, match="fp32"):
        D.decode_features(x, img, (8, 8), compute="bf16x3", initq=img)
    with pytest.raises(ValueError, match="fp32"):
        D.decode_features(x, img, (8, 8), compute="bf16", initq=img, initq_x3=img)
    with pytest.raises(NotImplementedError, match="mode 3"):
        D.decode_features(x, img, (8, 8), mode=2, compute="bf16x3", initq=img, initq_x3=img)
    with pytest.raises(ValueError, match="initq_x3"):
        D.decode_features(x, img, (8, 8), initq=img, initq_x3=img)
    with pytest.raises(ValueError, match="initq_x3"):
        D.decode_features(x, img, (8, 8), compute="bf16x3", initq_x3=img)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        D.decode_features(x, img, (8, 8), compute="bf16x3", initq=img, initq_x3=img)


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["b3_7x5_23x18", "b2_17x33_40x100_gain3", "siren_9x14_36x56"])
def test_planes_against_a_float64_product_of_the_fp32_operands(gold, dev, name):
    import diinn_amd._native as N
    import diinn_amd.decoder as D
    lib = N.load()
    _, b, h, w, hu, wu, gain, fgain = _case(gold, name)
    sd = _state_dict(gain, fgain)
    packed, image, image_x3 = _images(sd, dev)
    feat = torch.from_numpy(synth.encoder_features(123, b, h, w)).to(dev)
    pix = torch.full((b, hu * wu, 1280), float("nan"), device=dev)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    stream = torch.cuda.current_stream().cuda_stream
    N.check(lib.diinn_initq_planes_x3(C.c_void_p(stream), ptr(feat), ptr(packed), ptr(image), ptr(image_x3), ptr(pix),
                                      b, h, w, hu, wu, 0, hu, N.SIN_ACCURATE), "diinn_initq_planes_x3")
    torch.cuda.synchronize()
    f64 = D.initq_planes_reference(sd, feat, (hu, wu), "f64")
    emu = D.initq_planes_reference(sd, feat, (hu, wu), "split").double()
    assert torch.isfinite(pix).all()
    for lo, hi, what in ((0, 1024, "Wx . x' + bK"), (1024, 1280, "Q0 . E + bQ0")):
        e_gpu = float((pix[..., lo:hi].double() - f64[..., lo:hi]).abs().max())
        e_emu = float((emu[..., lo:hi] - f64[..., lo:hi]).abs().max())
        print(f"{name} {what}: max|gpu - f64| = {e_gpu:.3e}, max|emulated split - f64| = {e_emu:.3e}, ratio {e_gpu / e_emu:.2f} "
              f"(max|f64| = {float(f64[..., lo:hi].abs().max()):.2f})")
        assert e_gpu <= PLANES_FACTOR * e_emu, (what, e_gpu, e_emu)
    # E and Q0 . E do not depend on the batch item
    for i in range(1, b):
        assert torch.equal(pix[i, :, 1024:], pix[0, :, 1024:])


@pytest.mark.gpu
@pytest.mark.parametrize("sin_mode", [0, 1, 2])
def test_reference_fixtures(gold, dev, sin_mode):
    noise = _noise(gold)
    bad = []
    for name, b, h, w, hu, wu, gain, fgain in _cases(gold):
        dec = _module(_state_dict(gain, fgain), dev, sin_mode=sin_mode)
        feat = torch.from_numpy(synth.encoder_features(123, b, h, w)).to(dev)
        with torch.no_grad():
            got = dec(feat, (hu, wu)).cpu().numpy()
        ref32 = gold[f"out/{name}"]
        ref64 = ref32.astype(np.float64) + gold[f"d64/{name}"].astype(np.float64)
        err = float(np.abs(got - ref32).max())
        e64 = float(np.abs(got - ref64).max())
        print(f"sin_mode {sin_mode} {name}: max|hip - ref32| = {err:.3e} (contract {_tol(ref32):.2e}); "
              f"max|hip - ref64| = {e64:.3e} = {e64 / noise[gain]:.2f} N (N = {noise[gain]:.3e})")
        if not err <= _tol(ref32):
            bad.append(f"{name}: {err:.3e} > {_tol(ref32):.2e}")
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["small4x3_110x9", "b2_17x33_40x100_gain3"])
def test_chunks_of_eight_rows_change_no_bit(gold, dev, monkeypatch, name):
    import diinn_amd.decoder as D
    _, b, h, w, hu, wu, gain, fgain = _case(gold, name)
    dec = _module(_state_dict(gain, fgain), dev)
    feat = torch.from_numpy(synth.encoder_features(123, b, h, w)).to(dev)
    with torch.no_grad():
        whole = dec(feat, (hu, wu)).clone()
    assert D.initq_chunk_rows(b, wu, dec.INITQ_CHUNK_BYTES) >= hu            # one chunk above
    monkeypatch.setattr(D.ImplicitDecoder, "INITQ_CHUNK_BYTES", 1)
    assert D.initq_chunk_rows(b, wu, dec.INITQ_CHUNK_BYTES) == 8 < hu
    dec._pix_workspaces.clear()
    with torch.no_grad():
        chunked = dec(feat, (hu, wu), 30000)
    assert next(iter(dec._pix_workspaces.values())).numel() == b * 8 * wu * 1280
    assert torch.equal(whole, chunked)
    assert float(np.abs(whole.cpu().numpy() - gold[f"out/{name}"]).max()) <= _tol(gold[f"out/{name}"])


@pytest.mark.gpu
def test_row_bands_are_bit_equal_and_write_nothing_else(gold, dev):
    import diinn_amd.decoder as D
    _, b, h, w, hu, wu, gain, fgain = _case(gold, "b3_7x5_23x18")            # Wu = 18: no multiple of either kernel's tile width
    sd = _state_dict(gain, fgain)
    packed, image, image_x3 = _images(sd, dev)
    feat = torch.from_numpy(synth.encoder_features(123, b, h, w)).to(dev)
    kw = dict(initq=image, initq_x3=image_x3, compute="bf16x3")
    full = D.decode_features(feat, packed, (hu, wu), **kw)
    assert float(np.abs(full.cpu().numpy() - gold["out/b3_7x5_23x18"]).max()) <= _tol(gold["out/b3_7x5_23x18"])
    for y0, y1 in ((0, 3), (3, 13), (13, 23), (5, 6), (9, 22)):              # off multiples of 8 at both ends
        out = torch.full((b, 3, hu, wu), -7.25, device=dev)
        got = D.decode_features(feat, packed, (hu, wu), out=out, rows=(y0, y1), **kw)
        assert got is out
        assert torch.equal(out[:, :, y0:y1], full[:, :, y0:y1]), (y0, y1)
        keep = torch.ones(hu, dtype=torch.bool, device=dev)
        keep[y0:y1] = False
        assert bool((out[:, :, keep] == -7.25).all()), (y0, y1)
    # the fp32 arithmetic through the same entry is another result, and the split image does not leak into it
    f32 = D.decode_features(feat, packed, (hu, wu), initq=image)
    assert not torch.equal(f32, full)


@pytest.mark.gpu
def test_one_nan_feature_reaches_exactly_the_pixels_the_fp32_path_makes_non_finite(gold, dev):
    _, b, h, w, hu, wu, gain, fgain = _case(gold, "b2_12x10_31x27_gain2")
    sd = _state_dict(gain, fgain)
    dec = _module(sd, dev)
    dec32 = _module(sd, dev, compute="f32")
    feat = torch.from_numpy(synth.encoder_features(123, b, h, w)).to(dev)
    bad = feat.clone()
    bad[1, 37, 5, 9] = float("nan")
    with torch.no_grad():
        clean = dec(feat, (hu, wu)).clone()
        got = dec(bad, (hu, wu)).cpu()
        want = ~torch.isfinite(dec32(bad, (hu, wu))).cpu()
    assert 0 < int(want.sum()) < want.numel()
    assert torch.equal(~torch.isfinite(got), want)
    assert torch.equal(got[~want], clean.cpu()[~want])


@pytest.mark.gpu
def test_a_split_image_without_its_validity_word_gives_nan_everywhere(gold, dev):
    import diinn_amd.decoder as D
    _, b, h, w, hu, wu, gain, fgain = _case(gold, "b3_7x5_23x18")
    sd = _state_dict(gain, fgain)
    packed, image, image_x3 = _images(sd, dev)
    feat = torch.from_numpy(synth.encoder_features(123, b, h, w)).to(dev)
    good = D.decode_features(feat, packed, (hu, wu), initq=image, initq_x3=image_x3, compute="bf16x3")
    assert torch.isfinite(good).all()
    broken = image_x3.clone()
    broken[4 * 4 * 9 * 2 * 2 * 256 + 256] = 0.0
    out = D.decode_features(feat, packed, (hu, wu), initq=image, initq_x3=broken, compute="bf16x3")
    assert torch.isnan(out).all()


BIG = (2, 40, 56, 132, 185)


@pytest.mark.gpu
def test_a_shape_past_the_fixtures(dev):
    """B = 2, 40 x 56 -> 132 x 185 (a non-integer scale that differs per axis; 17 x 24 workgroups of the planes kernel per
    image): against ``initq_forward_reference`` in float64 on the device, within the contract."""
    import diinn_amd.decoder as D
    b, h, w, hu, wu = BIG
    sd = _state_dict(seed=7)
    feat = torch.from_numpy(synth.encoder_features(7, b, h, w)).to(dev)
    with torch.no_grad():
        r64 = D.initq_forward_reference(sd, feat, (hu, wu), torch.float64)
        r32 = D.initq_forward_reference(sd, feat, (hu, wu), torch.float32).double()
        got = _module(sd, dev)(feat, (hu, wu)).double()
    noise = float((r32 - r64).abs().max())
    err = float((got - r64).abs().max())
    print(f"max|hip - f64| = {err:.3e}, fp32 restatement vs f64 = {noise:.3e} ({err / noise:.2f} x)")
    assert err <= TOL * max(1.0, float(r64.abs().max()))


@pytest.mark.gpu
def test_whole_model_with_the_switch_and_set_split_bf16(dev):
    import diinn_amd.modules as M
    torch.manual_seed(5)
    lit = M.SRLitModule(arch="diinn", mode=3, init_q=True).to(dev).eval()
    x = torch.rand(1, 3, 12, 10, device=dev)
    size = (31, 27)
    with torch.no_grad():
        f32 = lit(x, size, 30000).clone()
        lit.net.decoder.hip_initq_split_bf16 = True
        lit.net.set_split_bf16()
        x3 = lit(x, size, 30000).clone()
        lit.net.set_split_bf16(False)
        back = lit(x, size, 30000)
    err = float((x3 - f32).abs().max())
    print(f"max|split bf16 - fp32| = {err:.3e} (contract {TOL * max(1.0, float(f32.abs().max())):.2e})")
    assert err <= TOL * max(1.0, float(f32.abs().max()))
    assert not torch.equal(x3, f32)                                          # another arithmetic did run
    assert torch.equal(back, f32)
