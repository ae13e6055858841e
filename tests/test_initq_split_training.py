"""``init_q=True``, mode 3, under autograd in split-bf16 arithmetic (``ImplicitDecoder.hip_autograd_initq_split_bf16``), CPU part:
  * the emulation sheet (``initq_split_training.split_forward_reference`` / ``split_backward_reference``: torch fp32, radians, every
    MFMA product of the path through ``sheets.split_matmul``) against the float64 formula sheet on nine shapes (SHAPES below), and
    against the REAL reference's .grad fixtures where its forward flips no gate;
  * dropping any one of the three products of ``dx'`` and ``t`` misses the bound initq_bwd_x3_kernel is held to;
  * the host packer of the init_q split training image against a numpy restatement of the documented layout;
  * the opt-in switch and what keeps refusing; the new entry points' argument checks.
GPU part: tests/test_initq_split_training_gpu.py.

Bounds (the project's own): forward 1e-4 x max(1, max|ref|); gradients GRAD_RTOL = 1e-4 relative per tensor; rectified gates that
differ from the float64 forward: at most max(1, ceil(1e-5 x 4 x 256 x N)) -- all FOUR layers count, k_0 comes from a split GEMM too."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import diinn_amd.synth as synth
from test_initq_training import CASE_NAMES, GRAD_RTOL, check_against_fixture, inputs, saved_planes

SEED = 123
# (B, H, W, Hu, Wu, gain) beside the five fixture cases
EXTRA = {"px1": (1, 1, 1, 1, 1, 1.0),
         "n65": (1, 2, 3, 5, 13, 1.0),            # one pixel past a 64-pixel unit
         "n143": (1, 5, 6, 13, 11, 1.0),          # five plane tiles, the last ragged, the last workgroup half empty
         "gain3": (1, 9, 14, 36, 56, 3.0)}
SHAPES = list(CASE_NAMES) + list(EXTRA)
# the fixture cases whose emulated forward flips no gate against the float64 forward (found by this file's forward test, printed
# there): only for these is an end-to-end gradient comparison meaningful (a flipped gate is a step in the gradient)
NO_FLIP_FIXTURES = ("b1_1x1_7x5", "b1_3x2_9x4", "b1_8x8_5x6_down")


def shape_inputs(name):
    """(sd, feat, r, (b, h, w, hu, wu)) as ``test_initq_training.inputs`` builds them, for the fixture cases and the extra shapes."""
    if name not in EXTRA:
        return inputs(name)                                      # (the fixture's own seed: its .grad arrays belong to it)
    b, h, w, hu, wu, gain = EXTRA[name]
    sd = synth.decoder_state_dict(SEED, float(gain), mode=3, init_q=True)
    feat = synth.encoder_features(SEED, b, h, w)
    r = synth.uniform(SEED, f"gradw:initq:{name}", (b, 3, hu, wu), 1.0)
    return sd, feat, r, (b, h, w, hu, wu)


def flip_cap(n):
    return max(1, math.ceil(1e-5 * 4 * 256 * n))


_ref64, _emu = {}, {}


def reference64(name):
    """(out, planes [4,2,256,N]) of the float64 forward; computed once per shape and left unchanged."""
    if name not in _ref64:
        sd, feat, r, (b, h, w, hu, wu) = shape_inputs(name)
        _ref64[name] = saved_planes(sd, feat, (hu, wu), torch.float64)
    return _ref64[name]


def emulation(name):
    if name not in _emu:
        import diinn_amd.initq_split_training as IS
        sd, feat, r, (b, h, w, hu, wu) = shape_inputs(name)
        _emu[name] = IS.split_forward_reference(sd, feat, (hu, wu))
    return _emu[name]


def forward_figures(name, out, acts):
    """(output error, planes error, gates that differ, cap) of fp32 ``out`` / ``acts`` against the float64 forward, both errors
    relative to max(1, max|ref|)."""
    out64, acts64 = reference64(name)
    e_out = float((out.double().cpu() - out64).abs().max()) / max(1.0, float(out64.abs().max()))
    e_pl = float((acts.double().cpu() - acts64).abs().max()) / max(1.0, float(acts64.abs().max()))
    flips = int(((acts[:, 0].cpu() > 0) != (acts64[:, 0] > 0)).sum())
    return e_out, e_pl, flips, flip_cap(acts.shape[-1])


def relative_errors(names, got, want):
    """[(name, max|got - want| / max|want|)] per tensor, ``want`` in float64."""
    res = []
    for n, g, w in zip(names, got, want):
        assert tuple(g.shape) == tuple(w.shape), n
        res.append((n, float((g.double().cpu() - w.cpu()).abs().max()) / max(float(w.abs().max()), 1e-30)))
    return res


# ---------------------------------------------------------------------------
# the emulation sheet
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", SHAPES)
def test_emulation_forward_against_float64(name):
    out, acts = emulation(name)
    e_out, e_pl, flips, cap = forward_figures(name, out, acts)
    print(f"{name}: out err {e_out:.2e}, planes err {e_pl:.2e}, gates that differ {flips} (cap {cap}) of {acts[:, 0].numel()}")
    assert e_out <= 1e-4 and e_pl <= 1e-4
    assert flips <= cap
    if name in NO_FLIP_FIXTURES:
        assert flips == 0


@pytest.mark.parametrize("name", SHAPES)
def test_emulation_backward_with_pinned_gates(name):
    """The sheet's own planes, upcast, through float64 ``backward_from_saved_initq``: all 20 parameter gradients and d feat of the
    split backward within 1e-4 relative."""
    import diinn_amd.initq_split_training as IS
    import diinn_amd.initq_training as IT
    sd, feat, r, (b, h, w, hu, wu) = shape_inputs(name)
    _, acts = emulation(name)
    params = [torch.from_numpy(sd[n]) for n in IT.INITQ_PARAM_NAMES]
    g, f = torch.from_numpy(r), torch.from_numpy(feat)
    d_feat, d_params = IS.split_backward_reference(g, f, acts, params, (hu, wu))
    w_feat, w_params = IT.backward_from_saved_initq(g.double(), f.double(), acts.double(), [p.double() for p in params], (hu, wu))
    errs = relative_errors(["feat"] + IT.INITQ_PARAM_NAMES, [d_feat] + d_params, [w_feat] + w_params)
    assert len(errs) == 21
    worst = max(errs, key=lambda t: t[1])
    print(f"{name}: worst pinned gradient {worst[0]} {worst[1]:.2e}")
    assert worst[1] <= GRAD_RTOL, worst


@pytest.mark.parametrize("name", CASE_NAMES)
def test_emulation_gradients_against_the_reference_fixtures(name):
    """End to end against the real reference's .grad arrays: every figure printed (check_against_fixture prints before it asserts);
    asserted at 1e-4 relative only where the emulated forward flips no gate."""
    import diinn_amd.initq_split_training as IS
    import diinn_amd.initq_training as IT
    sd, feat, r, (b, h, w, hu, wu) = shape_inputs(name)
    out, acts = emulation(name)
    flips = forward_figures(name, out, acts)[2]
    params = [torch.from_numpy(sd[n]) for n in IT.INITQ_PARAM_NAMES]
    d_feat, d_params = IS.split_backward_reference(torch.from_numpy(r), torch.from_numpy(feat), acts, params, (hu, wu))
    grads = {n: g.numpy() for n, g in zip(IT.INITQ_PARAM_NAMES, d_params)}
    print(f"{name}: gates that differ from the float64 forward: {flips}")
    if name in NO_FLIP_FIXTURES:
        assert flips == 0
        check_against_fixture(name, d_feat.numpy(), grads)
    else:
        try:
            check_against_fixture(name, d_feat.numpy(), grads)
        except AssertionError as e:                               # print-only: the kink argument of DESIGN.md 3.7f
            print(f"{name}: beyond 1e-4 with {flips} flipped gates (not asserted): {e}")


def bwd_kernel_reference(sd, feat, g_plain, size, product=torch.matmul, dtype=torch.float64):
    """What initq_bwd_kernel / initq_bwd_x3_kernel compute from gate gradients ``g_plain`` [4, 512, N] in tensor algebra of ``dtype``:
    {u, da, xp, e}, each [576, N]; the two reductions dx' and t through ``product(w_t, g)``."""
    import diinn_amd.initq_training as IT
    p = {k: torch.from_numpy(v).to(dtype).to(g_plain.device) for k, v in sd.items()}
    a, xc, _ = IT.embedding_planes(feat.to(dtype), p, size)
    e, cos_a = torch.sin(a), torch.cos(a)
    b = feat.shape[0]
    e, cos_a = e.repeat(1, b), cos_a.repeat(1, b)
    g = g_plain.to(dtype)
    wx = [p["K.0.0.weight"].reshape(256, 576)] + [p[f"K.{i}.0.weight"].reshape(256, 832)[:, 256:] for i in (1, 2, 3)]
    dxp = sum(product(wx[i].t().contiguous(), g[i, :256].contiguous()) for i in range(4))
    t = product(p["Q.0.0.weight"].reshape(256, 576).t().contiguous(), g[0, 256:].contiguous())
    return {"u": dxp * e, "da": (dxp * xc + t) * cos_a, "xp": e * xc, "e": e}


def test_dropping_any_one_of_the_three_products_misses_the_bound():
    """U and dA from the split products against float64 on n143 with random G: all three terms hold 1e-4 x max|ref| (the bound
    initq_bwd_x3_kernel is held to on the GPU); any two of them miss it."""
    import diinn_amd.initq_split_training as IS
    sd, feat, r, (b, h, w, hu, wu) = shape_inputs("n143")
    n = b * hu * wu
    g_plain = torch.randn((4, 512, n), generator=torch.Generator().manual_seed(5))
    f = torch.from_numpy(feat)
    want = bwd_kernel_reference(sd, f, g_plain, (hu, wu))
    for terms in ((0, 1, 2), (1, 2), (0, 2), (0, 1)):
        got = bwd_kernel_reference(sd, f, g_plain, (hu, wu), product=lambda w_t, g_: IS.split_product(w_t, g_, terms), dtype=torch.float32)
        errs = {k: float((got[k].double() - want[k]).abs().max()) / float(want[k].abs().max()) for k in ("u", "da")}
        print(f"terms {terms}: U {errs['u']:.2e}, dA {errs['da']:.2e}")
        if len(terms) == 3:
            assert errs["u"] <= 1e-4 and errs["da"] <= 1e-4
        else:
            assert errs["u"] > 1e-4 and errs["da"] > 1e-4, terms


# ---------------------------------------------------------------------------
# the init_q split training image
# ---------------------------------------------------------------------------
OFF_Q0X, OFF_WORD, OFF_WXT, OFF_Q0T, FLOATS = 589824, 737280, 737284, 1392644, 1556484


def _bf16(u16):
    return (u16.astype(np.uint32) << 16).view(np.float32)


def _bf16_rne(x):
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return ((u + (((u >> 16) & 1) + 0x7FFF)) & 0xFFFF0000).view(np.float32)


def host_images(sd):
    import diinn_amd.decoder as D
    import diinn_amd.initq_split_training as IS
    import diinn_amd.initq_training as IT
    body = D.pack_state_dict(D.initq_body_state_dict(sd), mode=3).numpy()
    train = IT.pack_initq_train(sd).numpy()
    return body, train, IS.pack_initq_split_host(body, train)


def natural_sections(img):
    """The four sections of the image in natural order, by the documented layout (include/diinn_hip.h): {name: [hi | lo, rows, cols]}."""
    u = img.view(np.uint16)
    def fwd(lo, og):                                             # [og][group 4][tap 9][mt 2][hi, lo][h 2][r 32][j 8] -> [hl][64 og + 32 mt + r][(16 group + 8 h + j) * 9 + tap]
        a = _bf16(u[2 * lo:2 * lo + og * 4 * 9 * 2 * 2 * 512]).reshape(og, 4, 9, 2, 2, 2, 32, 8)
        return a.transpose(4, 0, 3, 6, 1, 5, 7, 2).reshape(2, og * 64, 576)
    def bwd(lo, chunks):                                         # [wave 4][chunk][ks 16][mt 5][hi, lo][h 2][r 32][j 8] -> [hl][32 (5 wave + mt) + r][256 chunk + 16 ks + 8 h + j]
        a = _bf16(u[2 * lo:2 * lo + 4 * chunks * 16 * 5 * 2 * 512]).reshape(4, chunks, 16, 5, 2, 2, 32, 8)
        return a.transpose(4, 0, 3, 6, 1, 2, 5, 7).reshape(2, 640, chunks * 256)
    return {"wx": fwd(0, 16), "q0x": fwd(OFF_Q0X, 4), "wxt": bwd(OFF_WXT, 4), "q0t": bwd(OFF_Q0T, 1)}


def natural_weights(sd):
    wx = np.concatenate([sd["K.0.0.weight"].reshape(256, 576)] + [sd[f"K.{i}.0.weight"].reshape(256, 832)[:, 256:] for i in (1, 2, 3)], 0)
    q0 = sd["Q.0.0.weight"].reshape(256, 576)
    pad = lambda m: np.concatenate([m.T, np.zeros((64, m.shape[0]), np.float32)], 0)    # noqa: E731
    return {"wx": wx, "q0x": q0, "wxt": pad(wx), "q0t": pad(q0)}


def test_split_image_places_every_piece_where_the_layout_says():
    """Weights on a 16-bit grid (so that hi + lo is exact): every value of Wx and Q.0 sits, as a hi/lo pair, exactly where the
    documented layout says, in all four sections; rows 576..639 of the transposed operands are zero; the validity word is present;
    nothing is divided by 2 pi."""
    import diinn_amd._native as N
    from test_initq_training import random_image_tensors
    lib = N.load()
    assert lib.diinn_initq_split_train_floats() == FLOATS == OFF_Q0T + 4 * 16 * 5 * 512
    rng = np.random.default_rng(11)
    sd = random_image_tensors(rng)
    for k in sd:                                                 # 16 significant bits
        sd[k] = np.round(sd[k] * 2.0 ** 10).clip(-32000, 32000).astype(np.float32) * np.float32(2.0 ** -10)
    sd.update({"last_layer.weight": np.zeros((3, 256, 1, 1), np.float32), "last_layer.bias": np.zeros(3, np.float32)})
    for i in range(4):
        sd[f"K.{i}.0.bias"] = np.zeros(256, np.float32)
        sd.setdefault(f"Q.{i}.0.bias", np.zeros(256, np.float32))
        if i:
            sd[f"Q.{i}.0.weight"] = np.zeros((256, 256, 1, 1), np.float32)
    body, train, img = host_images(sd)
    assert img.shape == (FLOATS,)
    assert img[OFF_WORD:OFF_WORD + 1].view(np.uint32)[0] == N.INITQ_SPLIT_TRAIN_MAGIC == 0x44495153
    assert np.array_equal(img[OFF_WORD + 1:OFF_WORD + 4], np.zeros(3, np.float32))
    nat, want = natural_sections(img), natural_weights(sd)
    for k in nat:
        assert nat[k].shape[1:] == want[k].shape, k
        assert np.array_equal(nat[k][0] + nat[k][1], want[k]), k     # every value in its place, exact as a pair
        assert np.array_equal(nat[k][0], _bf16_rne(want[k])), k
    for k in ("wxt", "q0t"):
        assert not nat[k][:, 576:].any()


def test_split_image_rounds_to_nearest_even_and_keeps_16_bits():
    """On the synthetic decoder weights: hi == bf16_rne(v), lo == bf16_rne(v - hi) (round to nearest even) everywhere, and hi + lo
    reproduces v to 2^-16 relative."""
    sd = synth.decoder_state_dict(SEED, 1.0, mode=3, init_q=True)
    body, train, img = host_images(sd)
    nat, want = natural_sections(img), natural_weights(sd)
    for k in nat:
        hi, lo = nat[k]
        assert np.array_equal(hi, _bf16_rne(want[k])), k
        assert np.array_equal(lo, _bf16_rne(want[k] - hi)), k
        assert float(np.abs((hi.astype(np.float64) + lo) - want[k]).max()) <= 2.0 ** -16 * float(np.abs(want[k]).max())
        assert bool((np.abs((hi.astype(np.float64) + lo) - want[k]) <= 2.0 ** -16 * np.abs(want[k])).all()), k


# ---------------------------------------------------------------------------
# the switch
# ---------------------------------------------------------------------------
PARENT_TEXT = ("diinn_amd: autograd through the HIP decode path covers modes 1-3 in fp32 with init_q=False (mode 3 is the "
               "reference's final model, modes 1/2 its ablations); call mode 4, init_q=True or the bf16 path under "
               "torch.no_grad() (mode 4 in fp32 with init_q=False trains once ImplicitDecoder.hip_autograd_mode4 is set)")


def _outcome(**kw):
    """(exception type, text) of one call under autograd on a CPU tensor."""
    import diinn_amd.decoder as D
    dec = D.ImplicitDecoder(**kw)
    x = torch.zeros(1, 64, 2, 2, requires_grad=True)
    with pytest.raises(Exception) as e:
        dec(x, (4, 4))
    return type(e.value), str(e.value)


def test_switch_off_and_switch_alone_refuse_with_the_parents_text():
    import diinn_amd.decoder as D
    assert D.ImplicitDecoder.hip_autograd_initq_split_bf16 is False
    assert D.ImplicitDecoder(mode=3, init_q=True).hip_autograd_initq_split_bf16 is False
    base = dict(mode=3, init_q=True, compute="bf16x3")
    assert _outcome(**base) == (NotImplementedError, PARENT_TEXT)
    assert _outcome(hip_initq_split_bf16=True, **base) == (NotImplementedError, PARENT_TEXT)
    assert _outcome(hip_autograd_initq_split_bf16=True, **base) == (NotImplementedError, PARENT_TEXT)
    # the other training switches do not open it
    assert _outcome(hip_autograd=True, hip_autograd_split_bf16=True, hip_initq_split_bf16=True, **base) == (NotImplementedError, PARENT_TEXT)


def test_both_switches_reach_the_device_check():
    import diinn_amd.decoder as D
    kind, text = _outcome(mode=3, init_q=True, compute="bf16x3", hip_initq_split_bf16=True, hip_autograd_initq_split_bf16=True)
    assert kind is RuntimeError and "GPU" in text
    dec = D.ImplicitDecoder(mode=3, init_q=True, compute="bf16x3", hip_initq_split_bf16=True, hip_autograd_initq_split_bf16=True)
    assert dec._route(True) == "grad_initq_split" and dec._route(False) == "initq"
    assert D.ImplicitDecoder._GRAD_MODULES["grad_initq_split"] == "initq_split_training"
    assert D.ImplicitDecoder._AUTOGRAD_ROUTES[-3] == ("grad_initq_split", (3,), True, ("bf16x3",), ("hip_initq_split_bf16", "hip_autograd_initq_split_bf16"))


@pytest.mark.parametrize("kw", [dict(mode=1, compute="bf16x3"), dict(mode=2, compute="bf16x3"), dict(mode=4, compute="bf16x3"),
                                dict(mode=1, compute="bf16"), dict(mode=2, compute="bf16_full"), dict(mode=4, compute="bf16"),
                                dict(mode=3, compute="bf16"), dict(mode=3, compute="bf16_full"),
                                dict(mode=3, compute="f32"), dict(mode=3, compute="f32", hip_autograd=True),
                                dict(mode=3, compute="bf16x3", init_q=False), dict(mode=3, compute="bf16x3", init_q=False, hip_autograd_split_bf16=True),
                                dict(mode=2, compute="f32", hip_autograd_initq_modes=True)],
                         ids=lambda k: "-".join(f"{a}{b}" for a, b in k.items()))
def test_switch_on_changes_no_other_combination(kw):
    """With both switches on, every other (mode, init_q, compute) answers what it answers with the new switch off."""
    kw = {"init_q": True, "hip_initq_modes": True, "hip_initq_split_bf16": True, **kw}
    off = _outcome(**kw)
    on = _outcome(hip_autograd_initq_split_bf16=True, **kw)
    assert on == off
    if kw["init_q"] and kw["compute"] in ("bf16", "bf16_full", "bf16x3"):
        assert off[0] is NotImplementedError                     # modes 1, 2, 4 in any bf16 arithmetic; "bf16" / "bf16_full" on mode 3


def test_set_split_bf16_leaves_the_switch_alone():
    import diinn_amd.modules as M
    net = M.DIINN(mode=3, init_q=True).set_split_bf16()
    assert net.decoder.compute == "bf16x3"
    assert net.decoder.hip_autograd_initq_split_bf16 is False and net.decoder.hip_initq_split_bf16 is False
    with pytest.raises(NotImplementedError):
        M.DIINN(mode=3, init_q=True, graphs=True)


# ---------------------------------------------------------------------------
# argument checks (no device needed: every entry point validates before its first launch)
# ---------------------------------------------------------------------------
def test_new_entry_points_validate_their_arguments():
    import diinn_amd._native as N
    lib = N.load()
    p = C.c_void_p(4096)                                         # 16-byte aligned, never dereferenced: the checks come first
    odd = C.c_void_p(4100)
    assert lib.diinn_pack_initq_split_train_host(None, None, None) == N.ERR_INVALID_ARG
    assert lib.diinn_pack_initq_split_train(None, None, p, p) == N.ERR_INVALID_ARG
    assert lib.diinn_pack_initq_split_train(None, p, None, p) == N.ERR_INVALID_ARG
    assert lib.diinn_pack_initq_split_train(None, p, p, None) == N.ERR_INVALID_ARG
    assert lib.diinn_pack_initq_split_train(None, p, p, odd) == N.ERR_INVALID_ARG
    fwd, bwd = lib.diinn_decode_initq_train_fwd_x3, lib.diinn_initq_backward_x3
    good = [p] * 8
    for i in range(8):
        args = list(good)
        args[i] = None
        assert fwd(None, *args, 1, 2, 2, 4, 4, 2) == N.ERR_INVALID_ARG, i
        assert bwd(None, *args, 1, 2, 2, 4, 4) == N.ERR_INVALID_ARG, i
    for dims in ((0, 2, 2, 4, 4), (1, 0, 2, 4, 4), (1, 2, 0, 4, 4), (1, 2, 2, 0, 4), (1, 2, 2, 4, 0)):
        assert fwd(None, *good, *dims, 2) == N.ERR_INVALID_ARG, dims
        assert bwd(None, *good, *dims) == N.ERR_INVALID_ARG, dims
    for mode in (-1, 3):
        assert fwd(None, *good, 1, 2, 2, 4, 4, mode) == N.ERR_UNSUPPORTED
    for i in (1, 2, 3, 4, 5):                                    # packed, train image, split, init_q split, planes: 16-byte aligned
        args = list(good)
        args[i] = odd
        assert fwd(None, *args, 1, 2, 2, 4, 4, 2) == N.ERR_INVALID_ARG, i
    for i in (2, 3):                                             # train image, init_q split
        args = list(good)
        args[i] = odd
        assert bwd(None, *args, 1, 2, 2, 4, 4) == N.ERR_INVALID_ARG, i
    assert fwd(None, *good, 1, 2, 2, 50000, 50000, 2) == N.ERR_TOO_LARGE
    assert bwd(None, *good, 1, 2, 2, 50000, 50000) == N.ERR_TOO_LARGE
