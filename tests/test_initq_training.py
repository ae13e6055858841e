"""Training path of the decoder with ``init_q=True``, mode 3 (diinn.py:48-51,113-115,132-139 under autograd), CPU part:
``initq_training.backward_from_saved_initq`` (the formula sheet) fed with planes from ``decoder.initq_forward_reference``, against
the REAL reference's .grad fixtures (tests/golden/diinn_golden_initq_grad_<case>.npz); the training image's host packer and its
gather index; the opt-in switch and what keeps refusing; the new entry points' argument checks.  GPU part:
tests/test_initq_training_gpu.py."""
import ctypes as C
import glob
import os

import numpy as np
import pytest
import torch

import diinn_amd.synth as synth

HERE = os.path.dirname(os.path.abspath(__file__))
ROW_STRIDE = 8
PREFIX = "diinn_golden_initq_grad_"
CASE_FILES = sorted(glob.glob(os.path.join(HERE, "golden", PREFIX + "*.npz")))
CASE_NAMES = [os.path.basename(f)[len(PREFIX):-len(".npz")] for f in CASE_FILES]
GRAD_RTOL = 1e-4                                                 # the project's gradient bound (tests/test_training_modes12.py)


def test_fixture_cases_are_the_five_of_the_issue():
    assert sorted(CASE_NAMES) == sorted(["b2_12x10_31x27", "b1_9x14_36x56_gain2", "b1_8x8_5x6_down", "b1_1x1_7x5", "b1_3x2_9x4"])
    for f in CASE_FILES:
        assert os.path.getsize(f) < (1 << 20)
        g = np.load(f)
        # the generator's keep rule: the reference's own fp32 gradients within 1e-5 of max|float64|, every tensor
        for key in g.files:
            if key.startswith("d64/") and key != "d64/out":
                assert g[key][0] <= 1e-5 * g[key][1], (f, key, g[key])


_gold = {}


def gold(name):
    if name not in _gold:
        _gold[name] = np.load(os.path.join(HERE, "golden", f"{PREFIX}{name}.npz"))
    return _gold[name]


def inputs(name):
    b, h, w, hu, wu, gain, seed = gold(name)["meta"]
    b, h, w, hu, wu, seed = int(b), int(h), int(w), int(hu), int(wu), int(seed)
    sd = synth.decoder_state_dict(seed, float(gain), mode=3, init_q=True)
    feat = synth.encoder_features(seed, b, h, w)
    r = synth.uniform(seed, f"gradw:initq:{name}", (b, 3, hu, wu), 1.0)
    return sd, feat, r, (b, h, w, hu, wu)


def strided(pname):
    return pname[0] in "KQ" and pname.endswith("weight")


def check_against_fixture(name, d_feat, grads, rtol=GRAD_RTOL):
    """max|g - ref| <= rtol * max|ref| per tensor (K and Q weights: every 8th output row is pinned).  Every figure is printed first."""
    g = gold(name)
    todo = [("feat", d_feat)] + list(grads.items())
    assert len(todo) == 21
    bad = []
    for pname, x in todo:
        ref = g[f"grad/{pname}"]
        if strided(pname):
            x = x[::ROW_STRIDE]
        assert x.shape == ref.shape, (pname, x.shape, ref.shape)
        err, top = float(np.abs(x - ref).max()), float(np.abs(ref).max())
        print(f"{name} {pname}: err {err:.3e} / max|ref| {top:.3e} = {err / max(top, 1e-30):.2e}")
        if not err <= rtol * top:
            bad.append((pname, err, top))
    assert not bad, bad


@torch.no_grad()
def saved_planes(sd, feat, size, dtype=torch.float32):
    """(out, acts [4,2,256,N]) of ``decoder.initq_forward_reference``: what the training forward saves, as plain planes."""
    import diinn_amd.decoder as D
    planes = []
    out = D.initq_forward_reference(sd, torch.from_numpy(feat), size, dtype, planes=planes)
    acts = torch.stack([torch.stack([k.permute(1, 0, 2).reshape(256, -1), s.permute(1, 0, 2).reshape(256, -1)]) for k, s in planes])
    return out, acts


# ---------------------------------------------------------------------------
# the formula sheet
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASE_NAMES)
def test_backward_formulas_initq_on_cpu(name):
    """initq_training.backward_from_saved_initq on activations computed on the CPU by decoder.initq_forward_reference (fp32),
    against the real reference's gradients: max|g - ref| <= 1e-4 max|ref| per tensor."""
    import diinn_amd.initq_training as IT
    sd, feat, r, (b, h, w, hu, wu) = inputs(name)
    out, acts = saved_planes(sd, feat, (hu, wu))
    ref_out = gold(name)["out"]
    assert float(np.abs(out.numpy() - ref_out).max()) <= 1e-4 * max(1.0, float(np.abs(ref_out).max()))
    params = [torch.from_numpy(sd[n]) for n in IT.INITQ_PARAM_NAMES]
    d_feat, d_params = IT.backward_from_saved_initq(torch.from_numpy(r), torch.from_numpy(feat), acts, params, (hu, wu))
    for n, g in zip(IT.INITQ_PARAM_NAMES, d_params):
        assert tuple(g.shape) == IT.INITQ_PARAM_SHAPES[n], n
    assert sorted(IT.INITQ_PARAM_NAMES) == sorted(sd.keys())
    check_against_fixture(name, d_feat.numpy(), {n: g.numpy() for n, g in zip(IT.INITQ_PARAM_NAMES, d_params)})
    d_none, _ = IT.backward_from_saved_initq(torch.from_numpy(r), torch.from_numpy(feat), acts, params, (hu, wu), need_feat_grad=False)
    assert d_none is None


# ---------------------------------------------------------------------------
# the training image
# ---------------------------------------------------------------------------
def random_image_tensors(rng):
    sd = {"first_layer.0.weight": rng.standard_normal((576, 3, 1, 1)), "first_layer.0.bias": rng.standard_normal(576),
          "Q.0.0.weight": rng.standard_normal((256, 576, 1, 1)), "Q.0.0.bias": rng.standard_normal(256),
          "K.0.0.weight": rng.standard_normal((256, 576, 1, 1))}
    for i in (1, 2, 3):
        sd[f"K.{i}.0.weight"] = rng.standard_normal((256, 832, 1, 1))
    return {k: v.astype(np.float32) for k, v in sd.items()}


def test_pack_initq_train_places_every_value_where_the_layout_says():
    """A numpy restatement of the layout (include/diinn_hip.h "TRAINING IMAGE") on random positions of every part: the radians copy
    of the init_q image's layout, the transposed weights in initq_bwd_kernel's two-pass stream order, the padding rows, the word."""
    import diinn_amd._native as N
    import diinn_amd.decoder as D
    import diinn_amd.initq_training as IT
    lib = N.load()
    n_img = lib.diinn_initq_train_packed_floats()
    assert n_img == lib.diinn_initq_packed_floats() + 4 * 5 * 32 * 5 * 256 == 969220
    assert lib.diinn_initq_packed_floats() == 150020              # the init_q image keeps its size
    rng = np.random.default_rng(7)
    sd = random_image_tensors(rng)
    img = IT.pack_initq_train(sd).numpy()
    assert img.shape == (n_img,)
    fw, fb = sd["first_layer.0.weight"].reshape(576, 3), sd["first_layer.0.bias"]
    q0 = sd["Q.0.0.weight"].reshape(256, 576)
    wx = [sd["K.0.0.weight"].reshape(256, 576)] + [sd[f"K.{i}.0.weight"].reshape(256, 832)[:, 256:] for i in (1, 2, 3)]
    # F [4][576]: bit for bit the tensors (radians: nothing is scaled)
    for col in range(3):
        assert np.array_equal(img[col * 576:(col + 1) * 576], fw[:, col])
    assert np.array_equal(img[3 * 576:4 * 576], fb)
    # Q0W in the init_q image's own piece order, unscaled
    infer = D.pack_initq({**sd, "Q.0.0.bias": sd["Q.0.0.bias"]}).numpy()
    for _ in range(2000):
        mp, kg, t, lane, e = (int(rng.integers(k)) for k in (4, 72, 2, 64, 4))
        pos = 2304 + ((((mp * 72 + kg) * 2) + t) * 64 + lane) * 4 + e
        kk = 4 * kg + e
        assert img[pos] == q0[32 * (2 * mp + t) + (lane & 31), (2 * (kk % 32) + (lane >> 5)) * 9 + kk // 32]
        assert abs(infer[pos] - img[pos] / (2 * np.pi)) <= 1e-6 * abs(img[pos])       # the inference image: the same value / 2 pi
    off = 2304 + 147456
    assert np.array_equal(img[off:off + 256], sd["Q.0.0.bias"])
    assert IT.image_word() == off + 256
    assert img[off + 256:off + 257].view(np.uint32)[0] == N.INITQ_TRAIN_MAGIC == 0x44495154 != N.INITQ_MAGIC
    assert np.array_equal(img[off + 257:off + 260], np.zeros(3, np.float32))
    # WT [wave 4][pass 2][chunk 5][kg 32][mt 3 | 2][lane 64][e 4]
    base = off + 260
    seen_pad = 0
    for _ in range(6000):
        wave, ps, chunk, kg, lane, e = (int(rng.integers(k)) for k in (4, 2, 5, 32, 64, 4))
        nm = 2 if ps else 3
        mt = int(rng.integers(nm))
        pos = base + wave * 204800 + ps * (5 * 32 * 3 * 256) + (((chunk * 32 + kg) * nm + mt) * 64 + lane) * 4 + e
        n = 32 * (5 * wave + 3 * ps + mt) + (lane & 31)
        ch = 2 * (4 * kg + e) + (lane >> 5)
        if n >= 576:
            seen_pad += 1
            assert img[pos] == 0.0
        else:
            assert img[pos] == (q0 if chunk == 4 else wx[chunk])[ch, n], (wave, ps, chunk, kg, mt, lane, e)
    assert seen_pad > 100
    # every transposed weight appears exactly once: the section is Wx_0..3 and Q0 plus 64 zero rows per chunk
    assert np.isclose(np.sort(np.abs(img[base:]))[::-1][:5 * 256 * 576].astype(np.float64).sum(),
                      sum(np.abs(a).astype(np.float64).sum() for a in wx + [q0]), rtol=1e-9)


def test_gather_index_reproduces_the_host_packer_bit_for_bit():
    import diinn_amd._native as N
    import diinn_amd.initq_training as IT
    idx = IT.train_image_gather_index()
    assert idx.dtype == torch.int64 and idx.shape == (N.load().diinn_initq_train_packed_floats(),)
    rng = np.random.default_rng(11)
    sd = random_image_tensors(rng)
    host = IT.pack_initq_train(sd)
    flat = torch.cat([torch.from_numpy(sd[n]).reshape(-1) for n in IT.IMAGE_NAMES] + [torch.zeros(1)])
    assert int(idx.max()) == flat.numel() - 1                     # the appended zero: padding rows and the word's place
    got = flat.index_select(0, idx)
    word = IT.image_word()
    assert got[word] == 0.0
    got[word:word + 1].view(torch.int32).fill_(N.INITQ_TRAIN_MAGIC)
    assert torch.equal(got.view(torch.int32), host.view(torch.int32))
    # the body image of an init_q decoder gathers through mode 3's index with a zero Q0 table
    assert IT.INITQ_PARAM_NAMES[:2] == ["first_layer.0.weight", "first_layer.0.bias"] and len(IT.INITQ_PARAM_NAMES) == 20


# ---------------------------------------------------------------------------
# the switch
# ---------------------------------------------------------------------------
def test_switch_off_keeps_every_refusal_and_on_refuses_what_is_out_of_scope():
    import diinn_amd.decoder as D
    import diinn_amd.modules as M
    x = torch.zeros(1, 64, 4, 4)
    assert D.ImplicitDecoder.hip_autograd is False
    dec = D.ImplicitDecoder(mode=3, init_q=True)
    assert dec.hip_autograd is False
    # off: the exceptions of test_decoder_initq.py::test_refusals_touch_no_device
    with pytest.raises(NotImplementedError, match="autograd"):
        dec(x, (8, 8))
    with torch.no_grad(), pytest.raises(RuntimeError, match="ROCm GPU"):
        dec(x, (8, 8))
    # on: the supported call fails only for want of a GPU -- as a keyword and as a plain attribute
    for on in (D.ImplicitDecoder(mode=3, init_q=True, hip_autograd=True), dec):
        on.hip_autograd = True
        with pytest.raises(RuntimeError, match="ROCm GPU"):
            on(x, (8, 8))
        with pytest.raises(RuntimeError, match="ROCm GPU"):
            on(x.clone().requires_grad_(True), (8, 8), None)
        with pytest.raises(RuntimeError, match="ROCm GPU"):      # bsize given: the no_grad inference path, which wants a GPU too
            on(x, (8, 8), 30000)
    # on: modes 1 / 2 / 4 with init_q, the bf16 arithmetics and graph replay keep refusing, on CPU tensors
    for m in (1, 2, 4):
        with pytest.raises(NotImplementedError, match="init_q=True for mode 3"):
            D.ImplicitDecoder(mode=m, init_q=True, hip_autograd=True)(x, (8, 8))
    for comp in ("bf16", "bf16_full", "bf16x3"):
        bad = D.ImplicitDecoder(mode=3, init_q=True, compute=comp, hip_autograd=True)
        with pytest.raises(NotImplementedError, match="autograd"):
            bad(x, (8, 8))
        with torch.no_grad(), pytest.raises(ValueError, match="fp32 only"):
            bad(x, (8, 8))
    with pytest.raises(NotImplementedError, match="graph replay"):
        M.DIINN(3, True, graphs=True)
    # the switch has no effect with init_q=False: mode 4 under autograd refuses, mode 3 goes to its own training path
    with pytest.raises(NotImplementedError, match="autograd"):
        D.ImplicitDecoder(mode=4, hip_autograd=True)(x, (8, 8))
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        D.ImplicitDecoder(mode=3, hip_autograd=True)(x, (8, 8))
    # through the module: lit.net.decoder.hip_autograd = True
    lit = M.SRLitModule(arch="diinn", mode=3, init_q=True)
    with pytest.raises(NotImplementedError, match="autograd"):
        lit.net.decoder(x, (8, 8))
    lit.net.decoder.hip_autograd = True
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        lit.net.decoder(x, (8, 8))
    assert "hip_autograd" not in lit.state_dict() and not any("hip_autograd" in k for k in lit.state_dict())


def test_function_checks_its_arguments_before_any_device_work():
    import diinn_amd.initq_training as IT
    sd = synth.decoder_state_dict(123, 1.0, mode=3, init_q=True)
    params = [torch.from_numpy(sd[n]) for n in IT.INITQ_PARAM_NAMES]
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        IT.DecodeInitqFunction.apply(torch.zeros(1, 64, 2, 2), 4, 4, 2, *params)


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
    f = N.fptr
    buf = np.zeros(4, np.float32)
    k3 = N._f3(f(buf), f(buf), f(buf))
    assert lib.diinn_pack_initq_train(None, f(buf), f(buf), f(buf), f(buf), k3, f(buf)) == INV
    assert lib.diinn_pack_initq_train(f(buf), f(buf), f(buf), f(buf), None, k3, f(buf)) == INV
    assert lib.diinn_pack_initq_train(f(buf), f(buf), f(buf), f(buf), f(buf), N._f3(f(buf), None, f(buf)), f(buf)) == INV
    assert lib.diinn_pack_initq_train(f(buf), f(buf), f(buf), f(buf), f(buf), k3, None) == INV
    fwd = lib.diinn_decode_initq_train_fwd
    good = [None, one, one, one, one, one, one, 1, 4, 4, 8, 8, 2]
    for i in range(1, 7):                                        # every pointer
        a = list(good)
        a[i] = None
        assert fwd(*a) == INV, i
    for i, v in ((7, 0), (8, 0), (9, 0), (10, 0), (11, 0)):      # empty maps
        a = list(good)
        a[i] = v
        assert fwd(*a) == INV, i
    for i in (2, 3, 4):                                          # misaligned images / planes
        a = list(good)
        a[i] = odd
        assert fwd(*a) == INV, i
    a = list(good)
    a[12] = 7
    assert fwd(*a) == N.ERR_UNSUPPORTED
    bwd = lib.diinn_initq_backward
    good = [None, one, one, one, one, one, one, one, 1, 4, 4, 8, 8]
    for i in range(1, 8):
        a = list(good)
        a[i] = None
        assert bwd(*a) == INV, i
    for i in (8, 9, 10, 11, 12):
        a = list(good)
        a[i] = 0
        assert bwd(*a) == INV, i
    for i in (2, 3):
        a = list(good)
        a[i] = odd
        assert bwd(*a) == INV, i
    cs = lib.diinn_cell_sum_rows
    good = [None, one, 576, 576, one, one, one, 1, 4, 4, 8, 8]
    for i in (1, 4, 5, 6):
        a = list(good)
        a[i] = None
        assert cs(*a) == INV, i
    for i in (7, 8, 9, 10, 11):
        a = list(good)
        a[i] = 0
        assert cs(*a) == INV, i
    assert cs(None, one, 576, 577, one, one, one, 1, 4, 4, 8, 8) == INV      # more rows summed than a tile has
    assert cs(None, one, 576, 0, one, one, one, 1, 4, 4, 8, 8) == INV
    assert cs(None, odd, 576, 576, one, one, one, 1, 4, 4, 8, 8) == INV
    fold = lib.diinn_fold3x3
    assert fold(None, None, one, 1, 64, 4, 4) == INV and fold(None, one, None, 1, 64, 4, 4) == INV
    for a in ((0, 64, 4, 4), (1, 0, 4, 4), (1, 64, 0, 4), (1, 64, 4, 0)):
        assert fold(None, one, one, *a) == INV
    assert fold(None, one, one, 1, 70000, 4, 4) == N.ERR_TOO_LARGE
