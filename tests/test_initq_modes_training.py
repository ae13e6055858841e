"""Training path of the decoder with ``init_q=True`` and modes 1, 2 and 4 (diinn.py:113-147 under autograd), CPU part:
``initq_modes_training.backward_from_saved_initq_modes`` (the formula sheet) in float64 on planes from
``forward_planes_initq_modes``, against the REAL reference's .grad fixtures (tests/golden/diinn_golden_initq_m<m>_grad_<case>.npz);
the switch matrix; the new entry points' argument checks; the gather indices of the images.  GPU part:
tests/test_initq_modes_training_gpu.py."""
import ctypes as C
import glob
import os

import numpy as np
import pytest
import torch

import diinn_amd.synth as synth

HERE = os.path.dirname(os.path.abspath(__file__))
GRAD_RTOL = 1e-4                                                 # the project's gradient bound (tests/test_training_modes12.py)
MODES = (1, 2, 4)
FOUR = ["b2_12x10_31x27", "b1_9x14_36x56_gain2", "b1_8x8_5x6_down", "b1_3x2_9x4"]
EXPECTED = {1: FOUR + ["b1_1x1_7x5"], 2: FOUR + ["b1_1x1_7x5"], 4: FOUR + ["b1_1x1_2x2"]}


def case_files(mode):
    return sorted(glob.glob(os.path.join(HERE, "golden", f"diinn_golden_initq_m{mode}_grad_*.npz")))


def case_name(path, mode):
    return os.path.basename(path)[len(f"diinn_golden_initq_m{mode}_grad_"):-len(".npz")]


CASES = [(m, case_name(f, m)) for m in MODES for f in case_files(m)]
_gold = {}


def gold(mode, name):
    if (mode, name) not in _gold:
        _gold[(mode, name)] = np.load(os.path.join(HERE, "golden", f"diinn_golden_initq_m{mode}_grad_{name}.npz"))
    return _gold[(mode, name)]


def inputs(mode, name):
    b, h, w, hu, wu, gain, seed, m, stride = gold(mode, name)["meta"]
    assert int(m) == mode
    b, h, w, hu, wu, seed = int(b), int(h), int(w), int(hu), int(wu), int(seed)
    sd = synth.decoder_state_dict(seed, float(gain), mode=mode, init_q=True)
    feat = synth.encoder_features(seed, b, h, w)
    r = synth.uniform(seed, f"gradw:initq_m{mode}:{name}", (b, 3, hu, wu), 1.0)
    return sd, feat, r, (b, h, w, hu, wu)


def strided(pname):
    return pname[0] in "KQ" and pname.endswith("weight")


def check_against_fixture(mode, name, d_feat, grads, rtol=GRAD_RTOL):
    """max|g - ref| <= rtol * max|ref| per tensor (K and Q weights: the fixture's row stride).  Every figure is printed first."""
    g = gold(mode, name)
    stride = int(g["meta"][8])
    todo = [("feat", d_feat)] + list(grads.items())
    assert len(todo) == 21
    bad = []
    for pname, x in todo:
        ref = g[f"grad/{pname}"]
        x = np.asarray(x)
        if strided(pname):
            x = x[::stride]
        assert x.shape == ref.shape, (pname, x.shape, ref.shape)
        err, top = float(np.abs(x - ref).max()), float(np.abs(ref).max())
        print(f"mode {mode} {name} {pname}: err {err:.3e} / max|ref| {top:.3e} = {err / max(top, 1e-30):.2e}")
        if not err <= rtol * top:
            bad.append((pname, err, top))
    assert not bad, bad


def test_fixture_cases_are_those_of_the_issue():
    for m in MODES:
        assert sorted(case_name(f, m) for f in case_files(m)) == sorted(EXPECTED[m])
        for f in case_files(m):
            assert os.path.getsize(f) < (1 << 20)
            g = np.load(f)
            assert int(g["meta"][6]) == (124 if (m, case_name(f, m)) == (4, "b1_9x14_36x56_gain2") else 123)
            for key in g.files:                                  # the generator's keep rule, every tensor
                if key.startswith("d64/") and key != "d64/out":
                    assert g[key][0] <= 1e-5 * g[key][1], (f, key, g[key])


# ---------------------------------------------------------------------------
# the formula sheet
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode,name", CASES)
def test_backward_formulas_in_float64_against_the_reference(mode, name):
    """forward_planes_initq_modes and backward_from_saved_initq_modes in float64 against the real reference's fp32 output and
    gradients: the output within 1e-4 max(1, max|ref|), every gradient within 1e-4 max|ref|."""
    import diinn_amd.initq_modes_training as MT
    sd, feat, r, (b, h, w, hu, wu) = inputs(mode, name)
    assert sorted(MT.INITQ_PARAM_NAMES) == sorted(sd.keys())
    shapes = MT.param_shapes(mode)
    params = [torch.from_numpy(sd[n]).double() for n in MT.INITQ_PARAM_NAMES]
    for n, t in zip(MT.INITQ_PARAM_NAMES, params):
        assert tuple(t.shape) == shapes[n], n                    # the reference's own shapes
    f64 = torch.from_numpy(feat).double()
    with torch.no_grad():
        out, acts = MT.forward_planes_initq_modes(f64, params, (hu, wu), mode)
        assert acts.shape == (4, 2, 256, b * hu * wu) and acts.dtype == torch.float64
        ref_out = gold(mode, name)["out"]
        err = float(np.abs(out.numpy() - ref_out).max())
        print(f"mode {mode} {name} out: err {err:.3e} / max|ref| {float(np.abs(ref_out).max()):.3e}")
        assert err <= 1e-4 * max(1.0, float(np.abs(ref_out).max()))
        d_feat, d_params = MT.backward_from_saved_initq_modes(torch.from_numpy(r).double(), f64, acts, params, (hu, wu), mode)
        for n, g in zip(MT.INITQ_PARAM_NAMES, d_params):
            assert tuple(g.shape) == shapes[n], n
        check_against_fixture(mode, name, d_feat.numpy(), {n: g.numpy() for n, g in zip(MT.INITQ_PARAM_NAMES, d_params)})
        d_none, _ = MT.backward_from_saved_initq_modes(torch.from_numpy(r).double(), f64, acts, params, (hu, wu), mode, need_feat_grad=False)
        assert d_none is None


def test_forward_restatement_agrees_with_the_inference_formula_sheet():
    """forward_planes_initq_modes is decoder.initq_modes_forward_reference plus the saved planes: the same output in float64."""
    import diinn_amd.decoder as D
    import diinn_amd.initq_modes_training as MT
    for mode in MODES:
        sd, feat, _, (b, h, w, hu, wu) = inputs(mode, "b1_3x2_9x4")
        params = [torch.from_numpy(sd[n]).double() for n in MT.INITQ_PARAM_NAMES]
        out, _ = MT.forward_planes_initq_modes(torch.from_numpy(feat).double(), params, (hu, wu), mode)
        ref = D.initq_modes_forward_reference(sd, torch.from_numpy(feat), (hu, wu), mode, torch.float64)
        # two summation orders of float64 sums of up to 832 products: 832 x 2^-53 = 9e-14 of the sum of |terms| per sum, which
        # cancellation lets exceed the result a thousandfold at most here: 1e-10
        assert float((out - ref).abs().max()) <= 1e-10 * max(1.0, float(ref.abs().max()))
    with pytest.raises(ValueError, match="modes 1, 2 and 4"):
        MT.param_shapes(3)


# ---------------------------------------------------------------------------
# the images
# ---------------------------------------------------------------------------
def test_image_tensors_and_gather_indices():
    """The images of a step are gathers of mode-3-shaped tensors: mode 1 widened with zero feature columns, mode 4 with a zero 1x1
    head.  The two indices they go through are permutations of what they are built from (every source element used, the rest the
    appended zero)."""
    import diinn_amd.initq_modes_training as MT
    import diinn_amd.initq_training as IT
    import diinn_amd.training as T
    for mode in MODES:
        sd = synth.decoder_state_dict(123, 1.0, mode=mode, init_q=True)
        params = [torch.from_numpy(sd[n]) for n in MT.INITQ_PARAM_NAMES]
        p = MT.image_tensors(params, mode)
        for n in MT.INITQ_PARAM_NAMES:
            assert tuple(p[n].shape) == IT.INITQ_PARAM_SHAPES[n], (mode, n)
        for i in (1, 2, 3):
            k = p[f"K.{i}.0.weight"].reshape(256, 832)
            assert torch.equal(k[:, :256], torch.from_numpy(sd[f"K.{i}.0.weight"]).reshape(256, -1)[:, :256])
            if mode == 1:
                assert not k[:, 256:].any()
            else:
                assert torch.equal(k, torch.from_numpy(sd[f"K.{i}.0.weight"]).reshape(256, 832))
        if mode == 4:
            assert not p["last_layer.weight"].any() and not p["last_layer.bias"].any()
        else:
            assert torch.equal(p["last_layer.weight"], torch.from_numpy(sd["last_layer.weight"]))
    # the training image: every element of its sources but the q-columns of K.1..3, once -- Q.0.0.weight twice (the forward's A
    # operand and its transpose for initq_bwd_kernel)
    idx = IT.train_image_gather_index()
    total = sum(int(np.prod(IT.INITQ_PARAM_SHAPES[n])) for n in IT.IMAGE_NAMES)
    src = idx[idx < total]
    assert torch.unique(src).numel() == total - 3 * 256 * 256
    assert src.numel() == total - 3 * 256 * 256 + 256 * 576
    # the body image: mode 3's index; every element of the 18 tensors at least once, nothing outside them
    bidx = T.pack_gather_index(3)
    btotal = sum(int(np.prod(T.PARAM_SHAPES[n])) for n in T.PARAM_NAMES)
    assert int(bidx.max()) == btotal and int(bidx.min()) >= 0
    assert torch.unique(bidx[bidx < btotal]).numel() == btotal


# ---------------------------------------------------------------------------
# the switch
# ---------------------------------------------------------------------------
def test_switch_matrix():
    import diinn_amd.decoder as D
    import diinn_amd.modules as M
    x = torch.zeros(1, 64, 4, 4)
    assert D.ImplicitDecoder.hip_autograd_initq_modes is False
    for m in MODES:
        # off: today's refusals (tests/test_decoder_initq_modes.py)
        dec = D.ImplicitDecoder(mode=m, init_q=True)
        assert dec.hip_autograd_initq_modes is False
        with pytest.raises(NotImplementedError, match="init_q=True for mode 3"):
            dec(x, (8, 8))
        dec.hip_initq_modes = True
        with pytest.raises(NotImplementedError, match="inference only"):
            dec(x, (8, 8))
        for other in ("hip_autograd", "hip_autograd_mode4"):     # the other training switches still do not open it
            setattr(dec, other, True)
            with pytest.raises(NotImplementedError, match="inference only"):
                dec(x, (8, 8))
        # on alone: nothing changes
        alone = D.ImplicitDecoder(mode=m, init_q=True, hip_autograd_initq_modes=True)
        assert alone.hip_autograd_initq_modes is True and alone.hip_initq_modes is False
        with pytest.raises(NotImplementedError, match="init_q=True for mode 3"):
            alone(x, (8, 8))
        with torch.no_grad(), pytest.raises(NotImplementedError, match="init_q=True for mode 3"):
            alone(x, (8, 8))
        # on together with hip_initq_modes: only the device is missing -- as keywords and as plain attributes
        both = D.ImplicitDecoder(mode=m, init_q=True, hip_initq_modes=True, hip_autograd_initq_modes=True)
        alone.hip_initq_modes = True
        for on in (both, alone):
            with pytest.raises(RuntimeError, match="ROCm GPU"):
                on(x, (8, 8))
            with pytest.raises(RuntimeError, match="ROCm GPU"):
                on(x.clone().requires_grad_(True), (8, 8), None)
            with pytest.raises(RuntimeError, match="ROCm GPU"):  # bsize given / no_grad: the inference path, which wants a GPU too
                on(x, (8, 8), 30000)
            with torch.no_grad(), pytest.raises(RuntimeError, match="ROCm GPU"):
                on(x, (8, 8))
        # the bf16 arithmetics keep refusing
        for comp in ("bf16", "bf16_full", "bf16x3"):
            bad = D.ImplicitDecoder(mode=m, init_q=True, compute=comp, hip_initq_modes=True, hip_autograd_initq_modes=True)
            with pytest.raises(NotImplementedError, match="inference only"):
                bad(x, (8, 8))
            with torch.no_grad(), pytest.raises(ValueError, match="fp32 only"):
                bad(x, (8, 8))
    # mode 4 with a 1 x N output
    m4 = D.ImplicitDecoder(mode=4, init_q=True, hip_initq_modes=True, hip_autograd_initq_modes=True)
    for size in ((1, 8), (8, 1)):
        with pytest.raises(ValueError, match="at least 2 x 2"):
            m4(x, size)
    # no effect on mode 3 or init_q=False
    with pytest.raises(NotImplementedError, match="autograd"):
        D.ImplicitDecoder(mode=3, init_q=True, hip_initq_modes=True, hip_autograd_initq_modes=True)(x, (8, 8))
    with pytest.raises(NotImplementedError, match="autograd"):
        D.ImplicitDecoder(mode=4, hip_initq_modes=True, hip_autograd_initq_modes=True)(x, (8, 8))
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        D.ImplicitDecoder(mode=2, hip_initq_modes=True, hip_autograd_initq_modes=True)(x, (8, 8))
    # graph replay and the sharded forward keep refusing
    with pytest.raises(NotImplementedError, match="graph replay"):
        M.DIINN(2, True, graphs=True)
    # through the module: the two lines of the README
    lit = M.SRLitModule(arch="diinn", mode=2, init_q=True)
    lit.net.decoder.hip_initq_modes = True
    with pytest.raises(NotImplementedError, match="inference only"):
        lit.net.decoder(x, (8, 8))
    lit.net.decoder.hip_autograd_initq_modes = True
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        lit.net.decoder(x, (8, 8))
    assert not any("hip_autograd" in k for k in lit.state_dict())


def test_sharded_forward_keeps_refusing():
    import diinn_amd.modules as M
    for mode in MODES:
        net = M.DIINN(mode=mode, init_q=True)
        net.decoder.hip_initq_modes = True
        net.decoder.hip_autograd_initq_modes = True
        with pytest.raises(NotImplementedError, match="mode 4" if mode == 4 else "init_q"):
            net.forward_sharded(torch.zeros(1, 3, 4, 4), (8, 8))


def test_function_checks_its_arguments_before_any_device_work():
    import diinn_amd.initq_modes_training as MT
    for mode in MODES:
        sd = synth.decoder_state_dict(123, 1.0, mode=mode, init_q=True)
        params = [torch.from_numpy(sd[n]) for n in MT.INITQ_PARAM_NAMES]
        with pytest.raises(RuntimeError, match="ROCm GPU"):
            MT.DecodeInitqModesFunction.apply(torch.zeros(1, 64, 2, 2), 4, 4, 2, mode, *params)
    with pytest.raises(ValueError, match="at least 2 x 2"):
        MT.DecodeInitqModesFunction.apply(torch.zeros(1, 64, 2, 2), 1, 4, 2, 4, *params)
    with pytest.raises(ValueError, match="modes 1, 2 and 4"):
        MT.backward_fused_initq_modes(None, None, None, None, None, (4, 4), 3)


# ---------------------------------------------------------------------------
# C ABI: argument checks (no GPU: every call fails validation before its first launch)
# ---------------------------------------------------------------------------
def test_new_entry_points_reject_bad_arguments_without_a_gpu():
    import diinn_amd._native as N
    lib = N.load()
    assert lib.diinn_abi_version() == 11
    one = C.c_void_p(4096)                                       # never dereferenced
    odd = C.c_void_p(4100)                                       # not 16-byte aligned
    INV = N.ERR_INVALID_ARG
    fwd = lib.diinn_decode_initq_train_fwd_qonly
    for seeds in (0, 1):
        good = [None, one, one, one, one, one, one, 1, 4, 4, 8, 8, 2, seeds]
        for i in range(1, 7):                                    # every pointer
            a = list(good)
            a[i] = None
            assert fwd(*a) == INV, i
        for i in (7, 8, 9, 10, 11):                              # empty maps
            a = list(good)
            a[i] = 0
            assert fwd(*a) == INV, i
        for i in (2, 3, 4):                                      # misaligned images / planes
            a = list(good)
            a[i] = odd
            assert fwd(*a) == INV, i
        a = list(good)
        a[12] = 7
        assert fwd(*a) == N.ERR_UNSUPPORTED
        a = list(good)
        a[7], a[10], a[11] = 4, 20000, 20000                     # 1.6e9 HR pixels: past DIINN_TRAIN_MAX_PIXELS
        assert fwd(*a) == N.ERR_TOO_LARGE
        a = list(good)
        a[10], a[11] = 50000, 50000                              # an image of 2.5e9 pixels
        assert fwd(*a) == N.ERR_TOO_LARGE
    bwd = lib.diinn_pixel_chain_bwd
    good = [None, one, one, one, 143]
    for i in (1, 2, 3):
        a = list(good)
        a[i] = None
        assert bwd(*a) == INV, i
        a = list(good)
        a[i] = odd
        assert bwd(*a) == INV, i
    for n in (0, -5):
        assert bwd(None, one, one, one, n) == INV
    assert bwd(None, one, one, one, (1 << 30) + 1) == N.ERR_TOO_LARGE
