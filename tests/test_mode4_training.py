"""Training path of decoder mode 4, CPU part: the formula sheet (``mode4_training.backward_from_saved_mode4``) fed by the torch
restatement of the forward against the REAL reference's .grad fixtures (tests/golden/make_golden_grad_m4.py); the adjoint of the
reflect-padded gather against autograd; the device packer of the head image against the C ABI's; the refusals and the switch
``ImplicitDecoder.hip_autograd_mode4``; the argument checks of the two new entry points.  (GPU part: tests/test_mode4_training_gpu.py.)"""
import ctypes as C
import glob
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import diinn_amd.synth as synth

HERE = os.path.dirname(os.path.abspath(__file__))
PREFIX = os.path.join(HERE, "golden", "diinn_golden_grad_m4_")
ROW_STRIDE = 8
GRAD_RTOL = 1e-4                                    # the project's gradient contract (tests/test_training.py)
CASE_NAMES = ["c1x1_2x2", "row3x2_2x7", "col4x3_9x2", "b1_2x2_3x3", "b3_7x5_23x18", "b2_12x10_31x27_gain2", "down16x12_8x6",
              "b1_9x14_36x56_gain3"]

_gold = {}


def gold(name):
    if name not in _gold:
        _gold[name] = np.load(PREFIX + name + ".npz")
    return _gold[name]


def inputs(name):
    """(state dict, features, R = d loss / d out, (b, h, w, hu, wu)) regenerated as make_golden_grad_m4.py drew them."""
    b, h, w, hu, wu, gain, seed = gold(name)["meta"]
    b, h, w, hu, wu, seed = int(b), int(h), int(w), int(hu), int(wu), int(seed)
    sd = synth.decoder_state_dict(seed=seed, gain=float(gain), mode=4)
    feat = synth.encoder_features(seed, b, h, w)
    r = synth.uniform(seed, f"gradw:m4:{name}", (b, 3, hu, wu), 1.0)
    return sd, feat, r, (b, h, w, hu, wu)


def strided(pname):
    return pname[0] in "KQ" and pname.endswith("weight")


def check_against_fixture(name, d_feat, grads, rtol=GRAD_RTOL):
    """max|g - ref| <= rtol * max|ref| per tensor (K and Q weights: every 8th output row is pinned)."""
    g = gold(name)
    bad = []
    for pname, got in [("feat", d_feat)] + sorted(grads.items()):
        ref = g[f"grad/{pname}"]
        if strided(pname):
            got = got[::ROW_STRIDE]
        assert got.shape == ref.shape, (pname, got.shape, ref.shape)
        err, top = float(np.abs(got - ref).max()), float(np.abs(ref).max())
        print(f"{name} {pname}: err {err:.3e} / max|ref| {top:.3e} = {err / max(top, 1e-30):.2e}")
        if not err <= rtol * max(top, 1e-30):
            bad.append((pname, err, top))
    assert not bad, (name, bad)


def test_the_fixture_set_is_the_one_the_generator_writes():
    assert sorted(os.path.basename(p)[len("diinn_golden_grad_m4_"):-4] for p in glob.glob(PREFIX + "*.npz")) == sorted(CASE_NAMES)
    for name in CASE_NAMES:
        g = gold(name)
        assert os.path.getsize(PREFIX + name + ".npz") < 900_000
        # the reference's own fp32 gradients lie within 1e-5 of its float64 run for every tensor (the generator's cap)
        for key in g.files:
            if key.startswith("d64/") and key != "d64/out":
                d, top = g[key]
                assert d <= 1e-5 * top, (name, key, d, top)


# ---------------------------------------------------------------------------
# 1. the formula sheet against the fixtures
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASE_NAMES)
def test_formula_sheet_against_reference_fixtures(name):
    """forward_torch_mode4's planes -> backward_from_saved_mode4: every gradient within 1e-4 max|ref| of the real reference's
    .grad; the restated out within 1e-6 max(1, max|ref|) of the reference's."""
    import diinn_amd.mode4_training as M4
    import diinn_amd.training as T
    sd, feat, r, (b, h, w, hu, wu) = inputs(name)
    params = [torch.from_numpy(sd[n]) for n in T.PARAM_NAMES]
    for n, p_ in zip(T.PARAM_NAMES, params):
        assert tuple(p_.shape) == T.param_shapes(4)[n]
    with torch.no_grad():
        out, acts = M4.forward_torch_mode4(torch.from_numpy(feat), params, (hu, wu))
    ref = gold(name)["out"]
    err = float(np.abs(out.numpy() - ref).max())
    print(f"{name} out: err {err:.3e} / max|ref| {float(np.abs(ref).max()):.3e}")
    assert err <= 1e-6 * max(1.0, float(np.abs(ref).max()))
    d_feat, d_params = M4.backward_from_saved_mode4(torch.from_numpy(r), torch.from_numpy(feat), acts, params, (hu, wu))
    grads = {n: g.numpy() for n, g in zip(T.PARAM_NAMES, d_params)}
    for n in T.PARAM_NAMES:
        assert grads[n].shape == T.param_shapes(4)[n]
    check_against_fixture(name, d_feat.numpy(), grads)


def test_formula_sheet_in_float64_is_autograd_of_the_restated_forward():
    """The same sheet in float64 against autograd through forward_torch_mode4 in float64, every tensor in full: 1e-10 max|ref|
    (the sums are taken in other orders; the gates are measure-zero apart in float64)."""
    import diinn_amd.mode4_training as M4
    import diinn_amd.training as T
    sd, feat, r, (b, h, w, hu, wu) = inputs("b3_7x5_23x18")
    params = [torch.from_numpy(sd[n]).double().requires_grad_(True) for n in T.PARAM_NAMES]
    x = torch.from_numpy(feat).double().requires_grad_(True)
    out, acts = M4.forward_torch_mode4(x, params, (hu, wu))
    (out * torch.from_numpy(r).double()).sum().backward()
    d_feat, d_params = M4.backward_from_saved_mode4(torch.from_numpy(r).double(), x.detach(), acts.detach(),
                                                    [p_.detach() for p_ in params], (hu, wu))
    assert d_feat.dtype == torch.float64
    for n, got, want in [("feat", d_feat, x.grad)] + [(n, g, p_.grad) for n, g, p_ in zip(T.PARAM_NAMES, d_params, params)]:
        err, top = float((got - want).abs().max()), float(want.abs().max())
        assert err <= 1e-10 * top, (n, err, top)


# ---------------------------------------------------------------------------
# 2. the adjoint gather
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(2, 2), (2, 7), (9, 2), (3, 3), (5, 4)])
def test_adjoint_gather_is_autograd_of_reflect_pad_and_conv(hw):
    """dT = head_adjoint_taps(g): with T the tap image [B,27,Hu,Wu] (T[:, 3 k + c] = conv1x1 of q by Lw[c, :, ky, kx]) and
    out = the reflect-padded 9-point gather of T -- together F.pad(mode='reflect') + the 3x3 conv -- d <out, g> / d T equals dT,
    and through it the weight and input gradients of the conv itself; float64, 1e-12."""
    import diinn_amd.mode4_training as M4
    hu, wu = hw
    gen = torch.Generator().manual_seed(hu * 16 + wu)
    b, ch = 2, 5
    q = torch.randn((b, ch, hu, wu), generator=gen, dtype=torch.float64, requires_grad=True)
    lw = torch.randn((3, ch, 3, 3), generator=gen, dtype=torch.float64, requires_grad=True)
    g = torch.randn((b, 3, hu, wu), generator=gen, dtype=torch.float64)
    out = F.conv2d(F.pad(q, (1, 1, 1, 1), mode="reflect"), lw)
    (out * g).sum().backward()
    d_t = M4.head_adjoint_taps(g)                                                # [B, 27, Hu, Wu]
    assert tuple(d_t.shape) == (b, 27, hu, wu)
    # the gather written out: out[b, c, y, x] = sum_k T[b, 3 k + c, refl(y + ky - 1), refl(x + kx - 1)]; its adjoint by autograd
    t = torch.randn((b, 27, hu, wu), generator=gen, dtype=torch.float64, requires_grad=True)
    tp = F.pad(t, (1, 1, 1, 1), mode="reflect")
    gathered = sum(tp[:, 3 * (3 * ky + kx):3 * (3 * ky + kx) + 3, ky:ky + hu, kx:kx + wu] for ky in range(3) for kx in range(3))
    (gathered * g).sum().backward()
    assert float((d_t - t.grad).abs().max()) <= 1e-12
    # ... and carried through the 1x1 map: the conv's own gradients
    hrows = lw.detach().permute(2, 3, 0, 1).reshape(27, ch)
    d_q = torch.einsum("rc,brhw->bchw", hrows, d_t)
    d_lw = torch.einsum("brhw,bchw->rc", d_t, q.detach()).reshape(3, 3, 3, ch).permute(2, 3, 0, 1)
    assert float((d_q - q.grad).abs().max()) <= 1e-12 * max(1.0, float(q.grad.abs().max()))
    assert float((d_lw - lw.grad).abs().max()) <= 1e-12 * max(1.0, float(lw.grad.abs().max()))
    with pytest.raises(ValueError, match="2 x 2"):
        M4.head_adjoint_taps(torch.zeros(1, 3, 1, 4))


# ---------------------------------------------------------------------------
# 3. head packing
# ---------------------------------------------------------------------------
def test_pack_head3x3_on_device_is_the_host_packer_bit_for_bit():
    import diinn_amd._native as N
    import diinn_amd.decoder as D
    import diinn_amd.mode4_training as M4
    sd = synth.decoder_state_dict(7, 2.0, mode=4)
    want = D.pack_head3x3(sd)
    got = M4.pack_head3x3_on_device(torch.from_numpy(sd["last_layer.weight"]), torch.from_numpy(sd["last_layer.bias"]))
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(want.shape) == (N.load().diinn_head3x3_packed_floats(),)
    assert np.array_equal(got.numpy().view(np.uint32), want.numpy().view(np.uint32))
    assert int(got.numpy()[-1:].view(np.uint32)[0]) == N.HEAD3X3_MAGIC
    # the rows: r = 3 (3 ky + kx) + c
    lw = sd["last_layer.weight"]
    assert np.array_equal(got.numpy()[(3 * (3 * 2 + 1) + 2) * 256:(3 * (3 * 2 + 1) + 2) * 256 + 256], lw[2, :, 2, 1])
    with pytest.raises(ValueError, match="last_layer.weight"):
        M4.pack_head3x3_on_device(torch.zeros(3, 256, 1, 1), torch.zeros(3))


def test_layout_and_shapes_accept_mode_4():
    import diinn_amd.training as T
    assert T._layout(4) == 3 and T._layout(3) == 3 and T._layout(1) == 1
    with pytest.raises(ValueError):
        T._layout(5)
    s4 = T.param_shapes(4)
    assert s4["last_layer.weight"] == (3, 256, 3, 3)
    assert {k: v for k, v in s4.items() if k != "last_layer.weight"} == {k: v for k, v in T.PARAM_SHAPES.items() if k != "last_layer.weight"}
    assert T.param_shapes(3) is T.PARAM_SHAPES and T.PARAM_SHAPES["last_layer.weight"] == (3, 256, 1, 1)


# ---------------------------------------------------------------------------
# 4. refusals and the switch
# ---------------------------------------------------------------------------
def test_refusals_and_the_switch_without_a_gpu():
    import diinn_amd.decoder as D
    import diinn_amd.modules as M
    x = torch.zeros(1, 64, 4, 4)
    assert D.ImplicitDecoder.hip_autograd_mode4 is False
    dec = D.ImplicitDecoder(mode=4)
    assert dec.hip_autograd_mode4 is False
    # off: raises as before, and the message names the switch
    with pytest.raises(NotImplementedError, match="autograd") as e:
        dec(x, (8, 8))
    assert "hip_autograd_mode4" in str(e.value)
    with torch.no_grad(), pytest.raises(RuntimeError, match="ROCm GPU"):
        dec(x, (8, 8))
    # hip_autograd alone cannot serve
    with pytest.raises(NotImplementedError, match="autograd"):
        D.ImplicitDecoder(mode=4, hip_autograd=True)(x, (8, 8))
    # on: the supported call fails only for want of a GPU -- as a keyword and as a plain attribute
    dec.hip_autograd_mode4 = True
    for on in (D.ImplicitDecoder(mode=4, hip_autograd_mode4=True), dec):
        with pytest.raises(RuntimeError, match="ROCm GPU"):
            on(x, (8, 8))
        with pytest.raises(RuntimeError, match="ROCm GPU"):
            on(x.clone().requires_grad_(True), (8, 8), None)
        with pytest.raises(RuntimeError, match="ROCm GPU"):      # bsize given: the no_grad inference path, which wants a GPU too
            on(x, (8, 8), 30000)
        for size in ((1, 8), (8, 1)):                            # an output under 2 x 2: 'reflect' has nothing to reflect
            with pytest.raises(ValueError, match="2 x 2"):
                on(x, size)
    # on: bf16 computes and init_q keep refusing
    for comp in ("bf16", "bf16_full", "bf16x3"):
        with pytest.raises(NotImplementedError, match="autograd"):
            D.ImplicitDecoder(mode=4, compute=comp, hip_autograd_mode4=True)(x, (8, 8))
    with pytest.raises(NotImplementedError, match="init_q=True for mode 3"):
        D.ImplicitDecoder(mode=4, init_q=True, hip_autograd_mode4=True)(x, (8, 8))
    # the switch has no effect on the other modes: mode 3 goes to its own training path, init_q still wants its own switch
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        D.ImplicitDecoder(mode=3, hip_autograd_mode4=True)(x, (8, 8))
    with pytest.raises(NotImplementedError, match="autograd"):
        D.ImplicitDecoder(mode=3, init_q=True, hip_autograd_mode4=True)(x, (8, 8))
    # forward_sharded still does not cover mode 4; the switch is no parameter or buffer
    net = M.DIINN(mode=4, init_q=False)
    net.decoder.hip_autograd_mode4 = True
    with pytest.raises(NotImplementedError, match="mode 4"):
        net.forward_sharded(torch.zeros(1, 3, 4, 4), (8, 8))
    lit = M.SRLitModule(arch="diinn", mode=4)
    with pytest.raises(NotImplementedError, match="autograd"):
        lit.net.decoder(x, (8, 8))
    lit.net.decoder.hip_autograd_mode4 = True
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        lit.net.decoder(x, (8, 8))
    assert not any("hip_autograd" in k for k in lit.state_dict())


def test_function_checks_its_arguments_before_any_device_work():
    import diinn_amd.mode4_training as M4
    import diinn_amd.training as T
    sd = synth.decoder_state_dict(123, 1.0, mode=4)
    params = [torch.from_numpy(sd[n]) for n in T.PARAM_NAMES]
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        M4.DecodeMode4Function.apply(torch.zeros(1, 64, 2, 2), 4, 4, 2, *params)
    with pytest.raises(ValueError, match="2 x 2"):
        M4.DecodeMode4Function.apply(torch.zeros(1, 64, 2, 2), 1, 4, 2, *params)


# ---------------------------------------------------------------------------
# 5. C ABI: argument checks (no GPU: every call fails validation before its first launch)
# ---------------------------------------------------------------------------
def test_new_entry_points_reject_bad_arguments_without_a_gpu():
    import diinn_amd._native as N
    lib = N.load()
    assert lib.diinn_abi_version() == 11
    one = C.c_void_p(4096)                                       # never dereferenced
    odd = C.c_void_p(4100)                                       # not 16-byte aligned
    INV = N.ERR_INVALID_ARG
    fwd = lib.diinn_head3x3_from_planes
    good = [None, one, one, one, one, one, 1, 8, 8]
    for i in range(1, 6):                                        # every pointer
        a = list(good)
        a[i] = None
        assert fwd(*a) == INV, i
    for i, v in ((6, 0), (7, 1), (8, 1), (7, 0), (8, -3)):       # no batch; Hu = 1, Wu = 1: nothing to reflect
        a = list(good)
        a[i] = v
        assert fwd(*a) == INV, (i, v)
    for i in (1, 3, 4):                                          # misaligned planes / head image / tap buffer
        a = list(good)
        a[i] = odd
        assert fwd(*a) == INV, i
    a = list(good)
    a[6], a[7], a[8] = 4, 40000, 40000                           # B Hu Wu beyond the training path's pixel limit
    assert fwd(*a) == N.ERR_TOO_LARGE
    bwd = lib.diinn_backward_data_head3x3
    good = [None, one, one, one, one, one, one, one, 1, 8, 8]
    for i in range(1, 8):
        a = list(good)
        a[i] = None
        assert bwd(*a) == INV, i
    for i, v in ((8, 0), (9, 1), (10, 1), (9, 0), (10, -3)):
        a = list(good)
        a[i] = v
        assert bwd(*a) == INV, (i, v)
    a = list(good)
    a[8], a[9], a[10] = 4, 40000, 40000
    assert bwd(*a) == N.ERR_TOO_LARGE
