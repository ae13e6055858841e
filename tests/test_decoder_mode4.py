"""Decoder mode 4 (diinn.py:81-90, 140-147): mode 3 with last_layer = Conv2d(256, 3, 3, padding=1, padding_mode='reflect')
over the HR grid.  On the HIP path: decode_kernel<HEAD3> writes the 27 tap values of every pixel, head3x3_reflect_kernel
gathers nine of them per output (include/diinn_hip.h "decoder mode 4").

Fixtures: tests/golden/diinn_golden_r9.npz (tests/golden/make_golden_r9.py; the real reference in fp32 and, after
``.double()``, in float64).  Truth of a case: ref64 = out + d64.  The two bounds of the reference-parity test are those of
tests/test_decoder_modes.py, coded the same way: the 1e-4 contract, and FACTOR x N against ref64 with N = the largest
max|d64| over the cases of the same gain.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import diinn_amd.synth as synth

HERE = os.path.dirname(os.path.abspath(__file__))
TOL = 1e-4
FACTOR = 3.0                      # tests/test_decoder_modes.py
gpu = pytest.mark.gpu

# (name, b, h, w, hu, wu, gain): what make_golden_r9.py writes
R9_CASES = [("c1x1_2x2", 1, 1, 1, 2, 2, 1.0), ("row1x9_2x30", 1, 1, 9, 2, 30, 1.0), ("col13x3_40x2", 1, 13, 3, 40, 2, 1.0),
            ("b3_7x5_23x18", 3, 7, 5, 23, 18, 1.0), ("b2_12x10_31x27_gain2", 2, 12, 10, 31, 27, 2.0),
            ("down16x12_8x6", 1, 16, 12, 8, 6, 1.0), ("small4x3_110x9", 1, 4, 3, 110, 9, 1.0),
            ("b2_17x33_40x100_gain3", 2, 17, 33, 40, 100, 3.0)]


@pytest.fixture(scope="module")
def gold9():
    return np.load(os.path.join(HERE, "golden", "diinn_golden_r9.npz"))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return torch.device("cuda:0")


def _cases(g):
    for k in g.files:
        if k.startswith("meta/"):
            b, h, w, hu, wu, gain = g[k]
            yield k[5:], int(b), int(h), int(w), int(hu), int(wu), float(gain)


def _tol(ref):
    return TOL * max(1.0, float(np.abs(ref).max()))


def _images(sd, dev):
    import diinn_amd.decoder as D
    return D.pack_state_dict(sd, mode=4).to(dev), D.pack_head3x3(sd).to(dev)


def _decode(sd, feat, size, dev, **kw):
    import diinn_amd.decoder as D
    packed, head = _images(sd, dev)
    out = D.decode_features(torch.from_numpy(feat).to(dev), packed, size, mode=4, head=head, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _refl(i, n):
    return 1 if i < 0 else (n - 2 if i >= n else i)


# ---------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------
def test_synth_shapes_mode4_and_modes_1_to_3_unchanged():
    """``decoder_param_shapes(mode=4)`` is the reference's state_dict (3x3 head); tensors are drawn by name, so modes 1-3
    keep every bit (their head is U(+-1/16) over 768 values: the first of them pinned here) and mode 4 shares every K / Q
    tensor with mode 3."""
    import diinn_amd.decoder as D
    s4 = synth.decoder_param_shapes(mode=4)
    assert s4["last_layer.weight"] == (3, 256, 3, 3) and s4["last_layer.bias"] == (3,)
    dec = D.ImplicitDecoder(mode=4, init_q=False)
    assert {k: tuple(v.shape) for k, v in dec.state_dict().items()} == dict(s4)
    for mode in (1, 2, 3):
        assert synth.decoder_param_shapes(mode)["last_layer.weight"] == (3, 256, 1, 1)
        sd = synth.decoder_state_dict(123, mode=mode)
        assert sd["last_layer.weight"].shape == (3, 256, 1, 1)
        # the generator's own statement of the same tensor: name-keyed, bound 1/sqrt(fan_in = 256)
        assert np.array_equal(sd["last_layer.weight"], synth.uniform(123, "last_layer.weight", (3, 256, 1, 1), 1.0 / 16.0))
        assert np.array_equal(sd["last_layer.bias"], synth.uniform(123, "last_layer.bias", (3,), 1.0 / 16.0))
    sd3, sd4 = synth.decoder_state_dict(123, mode=3), synth.decoder_state_dict(123, mode=4)
    assert list(sd3) == list(sd4)
    for k in sd3:
        if not k.startswith("last_layer."):
            assert np.array_equal(sd3[k], sd4[k]), k
    assert sd4["last_layer.weight"].shape == (3, 256, 3, 3)
    assert float(np.abs(sd4["last_layer.weight"]).max()) <= 1.0 / 48.0            # fan_in 2304
    dec.load_state_dict({k: torch.from_numpy(v) for k, v in sd4.items()}, strict=True)


def test_pack_head3x3_layout():
    """[27][256]: row 3 (3 ky + kx) + c = Lw[c, :, ky, kx]; then Lb[3]; then the validity word."""
    import diinn_amd._native as N
    import diinn_amd.decoder as D
    lib = N.load()
    n = lib.diinn_head3x3_packed_floats()
    assert n == 27 * 256 + 4
    sd = synth.decoder_state_dict(7, mode=4)
    img = D.pack_head3x3(sd).numpy()
    assert img.shape == (n,)
    lw = sd["last_layer.weight"]
    want = np.ascontiguousarray(lw.transpose(2, 3, 0, 1)).reshape(27, 256)    # [ky][kx][c][ch]
    assert np.array_equal(img[:27 * 256].reshape(27, 256), want)
    assert np.array_equal(img[27 * 256:27 * 256 + 3], sd["last_layer.bias"])
    assert int(img[27 * 256 + 3:].view(np.uint32)[0]) == N.HEAD3X3_MAGIC
    assert lib.diinn_pack_head3x3(None, N.fptr(sd["last_layer.bias"]), N.fptr(img)) == N.ERR_INVALID_ARG
    # the body image: the mode-3 image of the same K / Q tensors with a zero 1x1 head section (sections 5 and 6)
    body = D.pack_state_dict(sd, mode=4).numpy()
    sd3 = dict(sd, **{"last_layer.weight": np.zeros((3, 256, 1, 1), np.float32), "last_layer.bias": np.zeros(3, np.float32)})
    assert np.array_equal(body.view(np.uint32), D.pack_state_dict(sd3, mode=3).numpy().view(np.uint32))
    off, size = C.c_size_t(), C.c_size_t()
    assert lib.diinn_packed_section(5, C.byref(off), C.byref(size)) == 0
    assert not body[off.value:off.value + size.value + 3].any()
    assert int(body[off.value + size.value + 3:].view(np.uint32)[0]) == N.PACKED_MAGIC


def test_mode4_rows_and_taps_bytes():
    import diinn_amd._native as N
    import diinn_amd.decoder as D
    lib = N.load()
    h, hu, wu = 12, 31, 27
    for (y0, y1), want in [((0, 1), (0, 2)), ((hu - 1, hu), (hu - 2, hu)), ((7, 8), (6, 9)), ((0, hu), (0, hu)),
                           ((7, 19), (6, 20))]:
        (ty0, ty1), (r0, r1) = D.mode4_rows(h, hu, wu, y0, y1)
        assert (ty0, ty1) == want
        assert (r0, r1) == D.lr_rows_for_band(h, hu, wu, ty0, ty1)
        for y in range(y0, y1):                                  # every reflected row of the band is in the buffer
            for ky in range(3):
                assert ty0 <= _refl(y + ky - 1, hu) < ty1
        assert lib.diinn_mode4_taps_bytes(2, hu, wu, y0, y1) == 2 * (ty1 - ty0) * wu * 28 * 4
    (ty0, ty1), _ = D.mode4_rows(1, 2, 2, 0, 1)
    assert (ty0, ty1) == (0, 2)
    a, b, c, d = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    refs = (C.byref(a), C.byref(b), C.byref(c), C.byref(d))
    assert lib.diinn_mode4_rows(4, 1, 8, 0, 1, *refs) == N.ERR_INVALID_ARG      # Hu < 2: the reference raises there too
    assert lib.diinn_mode4_rows(4, 8, 1, 0, 1, *refs) == N.ERR_INVALID_ARG      # Wu < 2
    assert lib.diinn_mode4_rows(4, 8, 8, 3, 3, *refs) == N.ERR_INVALID_ARG
    assert lib.diinn_mode4_rows(4, 8, 8, 0, 9, *refs) == N.ERR_INVALID_ARG
    assert lib.diinn_mode4_rows(4, 8, 8, 0, 8, None, C.byref(b), C.byref(c), C.byref(d)) == N.ERR_INVALID_ARG
    assert lib.diinn_mode4_taps_bytes(1, 1, 8, 0, 1) == 0 and lib.diinn_mode4_taps_bytes(1, 8, 8, 0, 9) == 0
    # the launch functions refuse the same shapes (and null pointers) before any launch
    one = C.c_void_p(16)
    assert lib.diinn_decode_mode4(None, one, one, one, one, one, one, 1, 4, 4, 1, 8, 0, 1, N.SIN_DEFAULT) == N.ERR_INVALID_ARG
    assert lib.diinn_decode_mode4_band(None, one, one, one, one, one, 1, 4, 4, 8, 1, 0, 8, N.SIN_DEFAULT) == N.ERR_INVALID_ARG
    assert lib.diinn_decode_mode4_band(None, one, one, None, one, one, 1, 4, 4, 8, 8, 0, 8, N.SIN_DEFAULT) == N.ERR_INVALID_ARG
    assert lib.diinn_decode_mode4(None, one, one, one, one, None, one, 1, 4, 4, 8, 8, 0, 8, N.SIN_DEFAULT) == N.ERR_INVALID_ARG
    assert lib.diinn_decode_mode4_band(None, one, one, one, one, one, 1, 4, 4, 8, 8, 0, 8, 7) == N.ERR_UNSUPPORTED


def test_fixture_file_keys_and_shapes(gold9):
    assert sorted(n for n, *_ in _cases(gold9)) == sorted(n for n, *_ in R9_CASES)
    assert len(gold9.files) == 3 * len(R9_CASES)
    for name, b, h, w, hu, wu, gain in R9_CASES:
        assert tuple(gold9[f"meta/{name}"]) == (b, h, w, hu, wu, gain)
        for kind in ("out", "d64"):
            a = gold9[f"{kind}/mode4/{name}"]
            assert a.shape == (b, 3, hu, wu) and a.dtype == np.float32 and np.isfinite(a).all()
        assert 0.0 < float(np.abs(gold9[f"d64/mode4/{name}"]).max()) < 1e-4


def test_tap_kernel_uses_no_scratch(tmp_path):
    """The three decode_kernel<SIN, true, false, HEAD3 = true> code objects of the shipped library: no scratch, no
    spilled register, one wave per SIMD, and the 27 KiB head table next to the Q0 rows in LDS (as
    tests/test_kernel_resources.py gates every kernel; here the mode-4 instantiations are picked out by name)."""
    import diinn_amd._native as N
    import test_kernel_resources as R
    if not os.path.exists(R.READELF):
        pytest.skip("llvm-readelf (ROCm) not installed")
    ks = R.kernel_metadata(N.LIB_PATH, tmp_path)
    taps = [k for k in ks if R.base_name(k[".name"]) == "decode_kernel" and k[".name"].endswith("ELb1ELb0ELb1EEv12DecodeParams")]
    assert len(taps) == 3, [k[".name"] for k in ks if "decode_kernel" in k[".name"]]
    for k in taps:
        assert int(k[".private_segment_fixed_size"]) == 0 and not k.get(".uses_dynamic_stack"), k[".name"]
        assert int(k[".vgpr_spill_count"]) == 0 and int(k[".sgpr_spill_count"]) == 0, k[".name"]
        assert int(k[".group_segment_fixed_size"]) == (3 + 27) * 256 * 4 + 16
        assert R.occupancy(k) >= 1
    (g,) = [k for k in ks if R.base_name(k[".name"]) == "head3x3_reflect_kernel"]
    assert int(g[".private_segment_fixed_size"]) == 0 and int(g[".vgpr_spill_count"]) == 0


def test_mode4_refusals_that_need_no_gpu():
    """Mode 4 under autograd raises NotImplementedError before anything looks at the device (like modes 1/2); under
    no_grad a CPU tensor keeps raising the "ROCm GPU" RuntimeError; ``forward_sharded`` does not cover mode 4."""
    import diinn_amd.decoder as D
    import diinn_amd.modules as M
    dec = D.ImplicitDecoder(mode=4, init_q=False)
    with pytest.raises(NotImplementedError, match="autograd"):
        dec(torch.zeros(1, 64, 4, 4), (8, 8))
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        with torch.no_grad():
            dec(torch.zeros(1, 64, 4, 4), (8, 8))
    with pytest.raises(NotImplementedError):
        D.ImplicitDecoder(mode=4, init_q=True)(torch.zeros(1, 64, 4, 4), (8, 8))
    net = M.DIINN(mode=4, init_q=False)
    with pytest.raises(NotImplementedError, match="mode 4"):
        net.forward_sharded(torch.zeros(1, 3, 4, 4), (8, 8))


# ---------------------------------------------------------------------------------------------------------------------
# GPU: reference parity
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("sin_mode", [0, 1, 2])
def test_reference_fixtures_at_the_noise_floor(gold9, dev, sin_mode):
    """Every r9 case against ref64 = out + d64, all three sine modes: the 1e-4 contract against ref32 and FACTOR x N
    against ref64 (both as in tests/test_decoder_modes.py).

    N (max|d64| per gain class): gain 1 9.5e-9, gain 2 7.4e-7, gain 3 1.3e-5.
    Measured on an MI355X (max|hip - ref64|, worst case of the class): sine mode 0: gain 1 1.5e-8 = 1.59 N (2x2 output
    2.9e-9), gain 2 8.6e-7 = 1.16 N, gain 3 1.1e-5 = 0.83 N; sine modes 1 and 2: gain 1 2.1e-8 = 2.24 N (small4x3_110x9),
    gain 2 9.2e-7 = 1.24 N, gain 3 1.3e-5 = 0.98 N.  Against ref32 the worst is 2.1e-5 at gain 3 (|ref| up to 5.6)."""
    mode = 4
    cases = list(_cases(gold9))
    N = {}
    for name, *_r, gain in cases:
        N[gain] = max(N.get(gain, 0.0), float(np.abs(gold9[f"d64/mode{mode}/{name}"]).max()))
    worst = {}
    for name, b, h, w, hu, wu, gain in cases:
        sd = synth.decoder_state_dict(123, gain, mode=mode)
        got = _decode(sd, synth.encoder_features(123, b, h, w), (hu, wu), dev, sin_mode=sin_mode)
        ref32 = gold9[f"out/mode{mode}/{name}"]
        ref64 = ref32.astype(np.float64) + gold9[f"d64/mode{mode}/{name}"].astype(np.float64)
        assert got.shape == ref32.shape
        err32 = float(np.abs(got - ref32).max())
        err64 = float(np.abs(got.astype(np.float64) - ref64).max())
        print(f"mode {mode} sin {sin_mode} {name}: N = {N[gain]:.3e}  max|hip - ref64| = {err64:.3e} = {err64 / N[gain]:.2f} N  "
              f"max|hip - ref32| = {err32:.3e}")
        worst[name] = (err64, N[gain])
        assert err32 <= _tol(ref32), f"{name}: contract {err32:.3e}"
    bad = {k: f"{e:.3e} > {FACTOR} x {n:.3e}" for k, (e, n) in worst.items() if e > FACTOR * n}
    assert not bad, f"mode {mode} sin_mode {sin_mode}: {bad}"


# ---------------------------------------------------------------------------------------------------------------------
# GPU: structure (no reference needed)
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("shape", [(1, 5, 4, 11, 13), (1, 3, 3, 2, 2)])
def test_single_tap_head_is_the_shifted_mode3_image(dev, shape):
    """Lb = 0 and head weights zero except tap (ky, kx), set to a mode-3 1x1 head L: mode 4 must equal this project's
    mode-3 decode of the same weights, reflect-padded by one and shifted by (ky, kx):
    out4[y, x] = out3[refl(y + ky - 1), refl(x + kx - 1)].  Pins the cross-correlation orientation, the tap order and both
    image edges.  The layers are the same code, only the two heads may round differently: tolerance 4 ulp of max|out3|
    (observed on an MI355X: 0, bit-equal, at both shapes and all nine taps)."""
    import diinn_amd.decoder as D
    b, h, w, hu, wu = shape
    sd3 = {k: v.copy() for k, v in synth.decoder_state_dict(41, mode=3).items()}
    sd3["last_layer.bias"][:] = 0.0
    L = sd3["last_layer.weight"].reshape(3, 256)
    feat = torch.from_numpy(synth.encoder_features(41, b, h, w)).to(dev)
    out3 = D.decode_features(feat, D.pack_state_dict(sd3, mode=3).to(dev), (hu, wu))
    scale = float(out3.abs().max())
    assert scale > 1e-3
    padded = F.pad(out3, (1, 1, 1, 1), mode="reflect")
    sd4 = dict(sd3)
    body = D.pack_state_dict(dict(sd4, **{"last_layer.weight": np.zeros((3, 256, 3, 3), np.float32)}), mode=4).to(dev)
    worst = 0.0
    for ky in range(3):
        for kx in range(3):
            lw = np.zeros((3, 256, 3, 3), np.float32)
            lw[:, :, ky, kx] = L
            sd4["last_layer.weight"] = lw
            out4 = D.decode_features(feat, body, (hu, wu), mode=4, head=D.pack_head3x3(sd4).to(dev))
            want = padded[:, :, ky:ky + hu, kx:kx + wu]
            # the same statement, index by index
            assert float(want[0, 1, 0, 0]) == float(out3[0, 1, _refl(ky - 1, hu), _refl(kx - 1, wu)])
            err = float((out4 - want).abs().max())
            worst = max(worst, err)
            assert err <= 4 * 2.0 ** -23 * scale, (ky, kx, err, scale)
    print(f"{shape}: max|out4 - shifted out3| = {worst:.3e} (max|out3| = {scale:.3e})")


@gpu
def test_zero_weights_give_the_bias_everywhere(dev):
    import diinn_amd.decoder as D
    sd = {k: v.copy() for k, v in synth.decoder_state_dict(5, mode=4).items()}
    sd["last_layer.weight"][:] = 0.0
    sd["last_layer.bias"][:] = np.array([0.25, -1.5, 3.0], np.float32)
    out = _decode(sd, synth.encoder_features(5, 2, 5, 4), (11, 13), dev)
    assert np.array_equal(out, np.broadcast_to(sd["last_layer.bias"].reshape(1, 3, 1, 1), out.shape))


@gpu
def test_row_bands_are_bit_equal_and_write_nothing_else(dev):
    """rows=(0,1), the last row, a middle band and a cover by chunks of 5 rows over ONE shared P workspace and ONE tap
    buffer: each band is bit-equal to the same rows of the whole-image decode and every other row of its NaN-filled
    ``out`` is still NaN (reflection is applied to image coordinates, never to band edges)."""
    import diinn_amd._native as N
    import diinn_amd.decoder as D
    b, h, w, hu, wu = 2, 12, 10, 31, 27
    sd = synth.decoder_state_dict(31, mode=4)
    packed, head = _images(sd, dev)
    feat = torch.from_numpy(synth.encoder_features(31, b, h, w)).to(dev)
    full = D.decode_features(feat, packed, (hu, wu), mode=4, head=head)
    assert bool(torch.isfinite(full).all())
    ws = torch.full((b * h * w * 1024,), float("nan"), device=dev)
    taps = torch.full((N.load().diinn_mode4_taps_bytes(b, hu, wu, 0, hu) // 4,), float("nan"), device=dev)
    bands = [(0, 1), (30, 31), (7, 19)]
    for y0, y1 in bands:
        out = torch.full((b, 3, hu, wu), float("nan"), device=dev)
        ret = D.decode_features(feat, packed, (hu, wu), out=out, workspace=ws, rows=(y0, y1), mode=4, head=head, taps=taps)
        torch.cuda.synchronize()
        assert ret is out
        assert torch.equal(out[:, :, y0:y1], full[:, :, y0:y1]), (y0, y1)
        assert bool(torch.isnan(out[:, :, :y0]).all()) and bool(torch.isnan(out[:, :, y1:]).all()), (y0, y1)
    cover = torch.full((b, 3, hu, wu), float("nan"), device=dev)
    for y0 in range(0, hu, 5):
        D.decode_features(feat, packed, (hu, wu), out=cover, workspace=ws, rows=(y0, min(hu, y0 + 5)), mode=4, head=head,
                          taps=taps)
    torch.cuda.synchronize()
    assert torch.equal(cover, full)
    with pytest.raises(ValueError):                              # a tap buffer that is too small is refused
        D.decode_features(feat, packed, (hu, wu), rows=(7, 19), mode=4, head=head, taps=taps[:100])
    with pytest.raises(ValueError):                              # and so is a decode without the head image
        D.decode_features(feat, packed, (hu, wu), mode=4)


@gpu
def test_c_abi_band_entry_point_and_validity_words(dev):
    """diinn_precompute_P on the rows diinn_mode4_rows reports, then diinn_decode_mode4_band: bit-equal to
    diinn_decode_mode4.  A head image without its validity word, or a body image without its own, answers NaN."""
    import diinn_amd._native as N
    import diinn_amd.decoder as D
    lib = N.load()
    b, h, w, hu, wu = 2, 12, 10, 31, 27
    sd = synth.decoder_state_dict(31, mode=4)
    packed, head = _images(sd, dev)
    feat = torch.from_numpy(synth.encoder_features(31, b, h, w)).to(dev)
    full = D.decode_features(feat, packed, (hu, wu), mode=4, head=head)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: C.c_void_p(t.data_ptr())                     # noqa: E731
    y0, y1 = 7, 19
    (ty0, ty1), (r0, r1) = D.mode4_rows(h, hu, wu, y0, y1)
    P = torch.full((b * h * w * 1024,), float("nan"), device=dev)
    N.check(lib.diinn_precompute_P_ex(stream, ptr(feat), ptr(packed), ptr(P), b, h, w, r0, r1, N.COMPUTE_F32), "P")
    taps = torch.empty(lib.diinn_mode4_taps_bytes(b, hu, wu, y0, y1) // 4, device=dev)
    out = torch.full((b, 3, hu, wu), float("nan"), device=dev)
    N.check(lib.diinn_decode_mode4_band(stream, ptr(P), ptr(packed), ptr(head), ptr(taps), ptr(out), b, h, w, hu, wu, y0, y1,
                                        N.SIN_DEFAULT), "band")
    torch.cuda.synchronize()
    assert torch.equal(out[:, :, y0:y1], full[:, :, y0:y1])
    assert bool(torch.isnan(out[:, :, :y0]).all()) and bool(torch.isnan(out[:, :, y1:]).all())
    bad_head = head.clone()
    bad_head[27 * 256 + 3] = 0.0
    assert bool(torch.isnan(D.decode_features(feat, packed, (hu, wu), mode=4, head=bad_head)).all())
    bad_body = packed.clone()
    off, size = C.c_size_t(), C.c_size_t()
    assert lib.diinn_packed_section(6, C.byref(off), C.byref(size)) == 0
    bad_body[off.value + 3] = 0.0
    assert bool(torch.isnan(D.decode_features(feat, bad_body, (hu, wu), mode=4, head=head)).all())


# ---------------------------------------------------------------------------------------------------------------------
# GPU: module level
# ---------------------------------------------------------------------------------------------------------------------
def _module(dev, seed=9, **kw):
    import diinn_amd.decoder as D
    sd = synth.decoder_state_dict(seed, mode=4)
    dec = D.ImplicitDecoder(mode=4, init_q=False, **kw).to(dev).eval()
    dec.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return dec, sd


@gpu
def test_module_forward_matches_decode_features(dev):
    """ImplicitDecoder(mode=4) under no_grad, every ``bsize`` (ignored: this path is the whole-image convolution), a
    second call through the cached images and workspaces, a changed parameter, and a side stream."""
    import diinn_amd.decoder as D
    dec, sd = _module(dev)
    b, h, w, hu, wu = 2, 7, 5, 23, 18
    feat = torch.from_numpy(synth.encoder_features(9, b, h, w)).to(dev)
    packed, head = _images(sd, dev)
    want = D.decode_features(feat, packed, (hu, wu), mode=4, head=head)
    with torch.no_grad():
        got = dec(feat, (hu, wu))
        assert torch.equal(got, want)
        assert torch.equal(dec(feat, [hu, wu], 30000), want) and torch.equal(dec(feat, (hu, wu), 7), want)
        assert len(dec._tap_workspaces) == 1 and torch.equal(dec.packed_head(dev), head)
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            on_side = dec(feat, (hu, wu))
        side.synchronize()
        assert torch.equal(on_side, want) and len(dec._tap_workspaces) == 2
        dec.last_layer.bias.add_(1.0)                            # the head image is re-packed with the body image
        assert torch.allclose(dec(feat, (hu, wu)), want + 1.0, rtol=0, atol=1e-6)
    with pytest.raises(NotImplementedError, match="autograd"):
        dec(feat, (hu, wu))
    with pytest.raises(ValueError):
        dec(feat, (hu, 1), 100)


@gpu
def test_chunked_forward_is_bit_equal_to_one_call(dev):
    """Hu = 300 > MODE4_CHUNK_ROWS = 254 on a narrow image: forward decodes rows [0,254) and [254,300) through a tap buffer
    of 256 rows (within the cap of 258); bit-equal to a single decode_features call over a 300-row tap buffer."""
    import diinn_amd._native as N
    import diinn_amd.decoder as D
    dec, sd = _module(dev)
    b, h, w, hu, wu = 1, 20, 3, 300, 6
    assert hu > dec.MODE4_CHUNK_ROWS and dec.MODE4_CHUNK_ROWS <= 256
    feat = torch.from_numpy(synth.encoder_features(9, b, h, w)).to(dev)
    packed, head = _images(sd, dev)
    want = D.decode_features(feat, packed, (hu, wu), mode=4, head=head)
    with torch.no_grad():
        got = dec(feat, (hu, wu))
    assert torch.equal(got, want)
    (taps,) = dec._tap_workspaces.values()
    assert taps.numel() * 4 == N.load().diinn_mode4_taps_bytes(b, hu, wu, 1, 255) == b * 256 * wu * 112


@gpu
def test_diinn_module_and_graph_replay(dev):
    """DIINN(mode=4): encoder + mode-4 decoder equals decode_features on the encoder's features; ``graphs=True`` replays to
    the same bits, also for new input contents; SRLitModule(arch="diinn", mode=4) builds the same net."""
    import diinn_amd.decoder as D
    import diinn_amd.modules as M
    torch.manual_seed(0)
    net = M.DIINN(mode=4, init_q=False).to(dev).eval()
    x, x2 = torch.rand(1, 3, 16, 12, device=dev), torch.rand(1, 3, 16, 12, device=dev)
    size = (37, 29)
    with torch.no_grad():
        feat = net.encoder(x)
        want = D.decode_features(feat, net.decoder.packed_weights(dev), size, mode=4, head=net.decoder.packed_head(dev))
        eager, eager2 = net(x, size), net(x2, size, 30000)
        assert torch.equal(eager, want)
        net.graphs = True
        assert torch.equal(net(x, size), eager) and torch.equal(net(x, size), eager)
        assert torch.equal(net(x2, size), eager2)
        assert len(net._graph_cache) == 1
    lit = M.SRLitModule(arch="diinn", mode=4)
    assert lit.net.decoder.mode == 4 and lit.net.decoder.last_layer.kernel_size == (3, 3)


# ---------------------------------------------------------------------------------------------------------------------
# GPU: refusals
# ---------------------------------------------------------------------------------------------------------------------
@gpu
def test_refusals(dev):
    import diinn_amd.decoder as D
    import diinn_amd.modules as M
    sd = synth.decoder_state_dict(3, mode=4)
    packed, head = _images(sd, dev)
    b, h, w, hu, wu = 1, 4, 4, 8, 8
    feat = torch.from_numpy(synth.encoder_features(3, b, h, w)).to(dev)
    for compute in ("bf16", "bf16_full", "bf16x3"):
        with pytest.raises(ValueError, match="fp32 only"):
            D.decode_features(feat, packed, (hu, wu), mode=4, head=head, compute=compute)
    dec, _ = _module(dev, compute="bf16")
    with pytest.raises(ValueError, match="fp32 only"):
        with torch.no_grad():
            dec(feat, (hu, wu))
    dec, _ = _module(dev)
    with pytest.raises(NotImplementedError, match="autograd"):
        dec(feat, (hu, wu))
    P = torch.zeros(b * h * w * 1024, device=dev)
    with pytest.raises(NotImplementedError, match="mode 4"):
        D.decode_tile(P, 0, (b, h, w), packed, (hu, wu), (0, 4), (0, 4), torch.zeros(b, 3, 4, 4, device=dev), mode=4)
    with pytest.raises(NotImplementedError, match="mode 4"):
        D.decode_window(feat, 0, h, packed, (hu, wu), (0, 4), mode=4)
    net = M.DIINN(mode=4, init_q=False).to(dev).eval()
    with pytest.raises(NotImplementedError, match="mode 4"):
        net.forward_sharded(torch.rand(1, 3, 8, 8, device=dev), (16, 16))
    with pytest.raises(ValueError):                              # Hu < 2: the reference raises there too
        D.decode_features(feat, packed, (1, 8), mode=4, head=head)
