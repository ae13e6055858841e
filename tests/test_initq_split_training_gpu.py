"""``init_q=True``, mode 3, under autograd in split-bf16 arithmetic, GPU part: ``diinn_decode_initq_train_fwd_x3``
(initq_planes_x3_kernel<SIN | INITQ_X3_RAD>, decode_bf16x3_kernel<SIN | X3_INITQ | X3_SAVE>), ``diinn_initq_backward_x3``
(initq_bwd_x3_kernel) and the device packer of the init_q split training image, against the float64 formula sheet; the mixed fp32 /
split forms; determinism; the validity word; a NaN feature; the switch through ``ImplicitDecoder.forward`` and ``SRLitModule``.
(CPU part, shapes, bounds and the float64 references: tests/test_initq_split_training.py.)"""
import ctypes as C

import numpy as np
import pytest
import torch

from test_initq_split_training import (GRAD_RTOL, SHAPES, bwd_kernel_reference, forward_figures, host_images, reference64,
                                       relative_errors, shape_inputs)

pytestmark = pytest.mark.gpu

SWITCHES = dict(compute="bf16x3", hip_initq_split_bf16=True, hip_autograd_initq_split_bf16=True)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def ptr(x):
    return C.c_void_p(x.data_ptr())


def decoder_for(sd, dev, **kw):
    import diinn_amd.decoder as D
    dec = D.ImplicitDecoder(mode=3, init_q=True, **kw)
    dec.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return dec.to(dev).train()


_fwd = {}


def forward_on_nan_planes(name, dev):
    """One split training forward per shape through the C ABI on NaN-filled buffers; computed once and left unchanged.
    Returns a dict: params, f, r, size, n, out, acts (tiled), plain [4,2,256,N], and the four images."""
    if name not in _fwd:
        import diinn_amd._native as N
        import diinn_amd.initq_split_training as IS
        import diinn_amd.initq_training as IT
        import diinn_amd.training as T
        lib = N.load()
        sd, feat, r, (b, h, w, hu, wu) = shape_inputs(name)
        params = [torch.from_numpy(sd[k]).to(dev) for k in IT.INITQ_PARAM_NAMES]
        f = torch.from_numpy(feat).to(dev)
        packed, image = IT.images_on_device(params)
        split, initq_split = IS.split_images_on_device(params)
        n = b * hu * wu
        nan = float("nan")
        acts = torch.full((4, (n + 31) // 32, 512, 32), nan, device=dev)
        out = torch.full((b, 3, hu, wu), nan, device=dev)
        pix = torch.full((lib.diinn_initq_pix_bytes(b, wu, hu) // 4,), nan, device=dev)
        st = lib.diinn_decode_initq_train_fwd_x3(C.c_void_p(torch.cuda.current_stream().cuda_stream), ptr(f), ptr(packed), ptr(image),
                                                 ptr(split), ptr(initq_split), ptr(pix), ptr(out), ptr(acts), b, h, w, hu, wu, N.SIN_DEFAULT)
        assert st == 0
        torch.cuda.synchronize()
        _fwd[name] = dict(sd=sd, params=params, f=f, r=torch.from_numpy(r).to(dev), size=(hu, wu), n=n, out=out, acts=acts,
                          plain=T.untile_planes(acts, n).reshape(4, 2, 256, n), packed=packed, image=image, split=split,
                          initq_split=initq_split)
    return _fwd[name]


@pytest.mark.parametrize("name", SHAPES)
def test_forward_on_nan_filled_planes(name, dev):
    """Output and planes within 1e-4 x max(1, max|ref|) of the float64 sheet, every element below N finite, the ragged tile's
    padding still NaN, flipped gates within the cap; the output within 1e-4 of the existing no-grad split inference on the same
    weights (radians here, revolutions there: close, not bit-equal)."""
    s = forward_on_nan_planes(name, dev)
    n, acts = s["n"], s["acts"]
    assert bool(torch.isfinite(s["out"]).all()) and bool(torch.isfinite(s["plain"]).all())
    if n % 32:
        assert bool(torch.isnan(acts[:, -1, :, n % 32:]).all()), "the padding of the ragged tile was written"
    e_out, e_pl, flips, cap = forward_figures(name, s["out"], s["plain"])
    print(f"{name}: out err {e_out:.2e}, planes err {e_pl:.2e}, gates that differ {flips} (cap {cap})")
    assert e_out <= 1e-4 and e_pl <= 1e-4
    assert flips <= cap
    dec = decoder_for(s["sd"], dev, compute="bf16x3", hip_initq_split_bf16=True)
    with torch.no_grad():
        infer = dec(s["f"], s["size"])
    d = float((infer - s["out"]).abs().max())
    ref = float(reference64(name)[0].abs().max())
    print(f"{name}: against the no-grad split inference {d:.2e} (max|ref| {ref:.2e})")
    assert d <= 1e-4 * max(1.0, ref)


def test_device_packer_is_the_host_twin_bit_for_bit(dev):
    s = forward_on_nan_planes("b1_3x2_9x4", dev)
    _, _, img = host_images(s["sd"])
    assert np.array_equal(s["initq_split"].cpu().numpy().view(np.uint32), img.view(np.uint32))


def test_initq_bwd_x3_kernel_alone(dev):
    """test_initq_bwd_kernel_alone's protocol on n143 (1 x 5 x 6 -> 13 x 11: five plane tiles in three workgroups, the last with one
    tile, that tile ragged): random G with NaN padding columns, a guard band behind every buffer.  U, dA against float64 tensor
    algebra to 1e-4 x max|ref| (three bf16 products leave about 2^-17 per operand pair; the emulation measures 5e-6), XP and E --
    fp32 by the forward's sequence -- to 1e-5 x max|ref|; padding rows exactly zero; padding columns and guard bands untouched."""
    import diinn_amd._native as N
    import diinn_amd.training as T
    lib = N.load()
    s = forward_on_nan_planes("n143", dev)
    sd, feat = s["sd"], s["f"]
    b, (hu, wu), n = 1, s["size"], s["n"]
    h, w = feat.shape[2:]
    t = (n + 31) // 32
    assert t == 5 and n % 32 == 15
    g_plain = torch.randn((4, 512, n), generator=torch.Generator().manual_seed(5))
    g_t = torch.stack([T.tile_planes(g_plain[i]) for i in range(4)]).to(dev)
    g_t[:, -1, :, n % 32:] = float("nan")
    guard, fill = 4096, -77.0
    sizes = {"u": 576, "da": 576, "xp": 640, "e": 640}
    bufs = {k: torch.full((t * rows * 32 + guard,), fill, device=dev) for k, rows in sizes.items()}
    st = lib.diinn_initq_backward_x3(C.c_void_p(torch.cuda.current_stream().cuda_stream), ptr(feat), ptr(g_t), ptr(s["image"]),
                                     ptr(s["initq_split"]), ptr(bufs["u"]), ptr(bufs["da"]), ptr(bufs["xp"]), ptr(bufs["e"]), b, h, w, hu, wu)
    assert st == 0
    torch.cuda.synchronize()
    want = bwd_kernel_reference(sd, feat, g_plain.to(dev), (hu, wu))
    bad = []
    for k, rows in sizes.items():
        assert bool((bufs[k][-guard:] == fill).all()), f"{k}: guard band written"
        tiled = bufs[k][:-guard].view(t, rows, 32)
        assert bool((tiled[-1, :, n % 32:] == fill).all()), f"{k}: padding columns of the ragged tile written"
        got = T.untile_planes(tiled, n)
        if rows == 640:
            assert bool((got[576:] == 0).all()), f"{k}: padding rows are not exactly zero"
        err, top = float((got[:576].double() - want[k]).abs().max()), float(want[k].abs().max())
        bound = 1e-4 if k in ("u", "da") else 1e-5
        print(f"{k}: err {err:.3e} / max {top:.3e} = {err / top:.2e} (bound {bound:.0e})")
        if not err <= bound * top:
            bad.append((k, err, top))
    assert not bad, bad


def all_split_backward(s):
    import diinn_amd.initq_training as IT
    return IT.backward_fused_initq(s["r"], s["f"], s["acts"], s["packed"], s["image"], s["size"], split=s["split"],
                                   initq_split=s["initq_split"])


@pytest.mark.parametrize("name", SHAPES)
def test_whole_backward_with_pinned_gates(name, dev):
    """The kernel's own saved planes, upcast, through float64 ``backward_from_saved_initq``: all 21 tensors within 1e-4 relative."""
    import diinn_amd.initq_training as IT
    s = forward_on_nan_planes(name, dev)
    d_feat, d_params = all_split_backward(s)
    w_feat, w_params = IT.backward_from_saved_initq(s["r"].double(), s["f"].double(), s["plain"].double(),
                                                    [p.double() for p in s["params"]], s["size"])
    errs = relative_errors(["feat"] + IT.INITQ_PARAM_NAMES, [d_feat] + d_params, [w_feat] + w_params)
    assert len(errs) == 21
    for pname, e in errs:
        print(f"{name} {pname}: {e:.2e}")
    bad = [(pname, e) for pname, e in errs if not e <= GRAD_RTOL]
    assert not bad, bad


@pytest.mark.parametrize("name", ["b2_12x10_31x27", "n65", "b1_8x8_5x6_down"])
def test_mixed_forms(name, dev):
    """On the split forward's planes: the fp32 backward; the fp32 chain with the split initq_backward_x3; the split chain with the
    fp32 initq_backward -- each within 1e-4 relative of the all-split result."""
    import diinn_amd.initq_training as IT
    s = forward_on_nan_planes(name, dev)
    a_feat, a_params = all_split_backward(s)
    ref = [a_feat.double()] + [g.double() for g in a_params]
    args = (s["r"], s["f"], s["acts"], s["packed"], s["image"], s["size"])
    forms = {"fp32 backward": {}, "fp32 chain, split initq_backward": dict(initq_split=s["initq_split"]),
             "split chain, fp32 initq_backward": dict(split=s["split"])}
    for label, kw in forms.items():
        d_feat, d_params = IT.backward_fused_initq(*args, **kw)
        errs = relative_errors(["feat"] + IT.INITQ_PARAM_NAMES, [d_feat] + d_params, ref)
        worst = max(errs, key=lambda t: t[1])
        print(f"{name}, {label}: worst {worst[0]} {worst[1]:.2e}")
        assert worst[1] <= GRAD_RTOL, (label, worst)


def test_two_passes_are_bit_identical(dev):
    import diinn_amd.initq_split_training as IS
    import diinn_amd.training as T
    s = forward_on_nan_planes("b2_12x10_31x27", dev)
    f1, g1 = all_split_backward(s)
    f2, g2 = all_split_backward(s)
    assert torch.equal(f1, f2)
    for a, b_ in zip(g1, g2):
        assert torch.equal(a, b_)
    out2, acts2 = IS.train_forward_initq_split(s["f"], s["params"], s["size"][0], s["size"][1], 2)[:2]
    assert torch.equal(out2, s["out"])
    assert torch.equal(T.untile_planes(acts2, s["n"]), T.untile_planes(s["acts"], s["n"]))


def test_an_image_without_its_validity_word_answers_nan(dev):
    import diinn_amd._native as N
    import diinn_amd.initq_training as IT
    import diinn_amd.initq_split_training as IS
    lib = N.load()
    s = forward_on_nan_planes("b1_3x2_9x4", dev)
    word = IS.image_word()
    assert int(s["initq_split"][word:word + 1].view(torch.int32)) == N.INITQ_SPLIT_TRAIN_MAGIC
    blank = s["initq_split"].clone()
    blank[word] = 0.0
    b, _, h, w = s["f"].shape
    hu, wu = s["size"]
    out, acts = torch.zeros_like(s["out"]), torch.zeros_like(s["acts"])
    pix = torch.zeros(lib.diinn_initq_pix_bytes(b, wu, hu) // 4, device=dev)
    st = lib.diinn_decode_initq_train_fwd_x3(C.c_void_p(torch.cuda.current_stream().cuda_stream), ptr(s["f"]), ptr(s["packed"]),
                                             ptr(s["image"]), ptr(s["split"]), ptr(blank), ptr(pix), ptr(out), ptr(acts), b, h, w, hu, wu, 2)
    assert st == 0
    assert bool(torch.isnan(out).all())
    d_feat, d_params = IT.backward_fused_initq(s["r"], s["f"], s["acts"], s["packed"], s["image"], s["size"], split=s["split"],
                                               initq_split=blank)
    named = dict(zip(IT.INITQ_PARAM_NAMES, d_params))
    assert bool(torch.isnan(d_feat).all())
    for pname in ("K.0.0.weight", "Q.0.0.weight", "first_layer.0.weight", "first_layer.0.bias"):
        assert bool(torch.isnan(named[pname]).all()), pname
    # and the inference entry points keep answering NaN on training images
    import diinn_amd.decoder as D
    infer = D.decode_features(s["f"], s["packed"], s["size"], initq=s["image"])
    assert bool(torch.isnan(infer).all())


def test_a_nan_feature_poisons_what_it_poisons_on_the_fp32_path(dev):
    """One NaN in feat (batch item 0, cell (6, 4) of 12 x 10): the non-finite pixels of the output and the non-finite entries of every
    gradient are exactly those of the fp32 training path."""
    import diinn_amd.initq_split_training as IS
    import diinn_amd.initq_training as IT
    s = forward_on_nan_planes("b2_12x10_31x27", dev)
    hu, wu = s["size"]
    f = s["f"].clone()
    f[0, 5, 6, 4] = float("nan")
    out_s, acts_s, packed, image, split, initq_split = IS.train_forward_initq_split(f, s["params"], hu, wu, 2)
    fs, gs = IT.backward_fused_initq(s["r"], f, acts_s, packed, image, s["size"], split=split, initq_split=initq_split)
    out_f, acts_f, _, _ = IT.train_forward_initq(f, s["params"], hu, wu, 2)
    ff, gf = IT.backward_fused_initq(s["r"], f, acts_f, packed, image, s["size"])
    assert bool((~torch.isfinite(out_s)).any()) and not bool((~torch.isfinite(out_s)).all())
    assert torch.equal(torch.isfinite(out_s), torch.isfinite(out_f))
    for pname, a, b_ in [("feat", fs, ff)] + list(zip(IT.INITQ_PARAM_NAMES, gs, gf)):
        assert torch.equal(torch.isfinite(a), torch.isfinite(b_)), pname


def test_through_the_decoder_with_the_switches_set(dev):
    """``ImplicitDecoder.forward`` under autograd with the three lines a user sets; with the new switch set, the no-grad output and
    the fp32 training gradients (compute="f32") are bit-identical to what they are with it unset."""
    s = forward_on_nan_planes("b2_12x10_31x27", dev)
    r = s["r"]

    def run(**kw):
        dec = decoder_for(s["sd"], dev, **kw)
        x = s["f"].clone().requires_grad_(True)
        out = dec(x, s["size"])
        assert out.requires_grad
        (out * r).sum().backward()
        with torch.no_grad():
            quiet = dec(x, s["size"])
        return out.detach(), x.grad, {n: p.grad for n, p in dec.named_parameters()}, quiet

    out, d_feat, grads, quiet = run(**SWITCHES)
    assert torch.equal(out, s["out"]) and len(grads) == 20
    a_feat, a_params = all_split_backward(s)
    assert torch.equal(d_feat, a_feat)
    off = decoder_for(s["sd"], dev, compute="bf16x3", hip_initq_split_bf16=True)
    with pytest.raises(NotImplementedError, match="autograd"):
        off(s["f"].clone().requires_grad_(True), s["size"])
    with torch.no_grad():
        assert torch.equal(off(s["f"], s["size"]), quiet)
    strips = decoder_for(s["sd"], dev, **SWITCHES)(s["f"].clone().requires_grad_(True), s["size"], 30000)
    assert not strips.requires_grad and torch.equal(strips, quiet)
    o1, f1, g1, q1 = run(compute="f32", hip_autograd=True)
    o2, f2, g2, q2 = run(compute="f32", hip_autograd=True, hip_initq_split_bf16=True, hip_autograd_initq_split_bf16=True)
    assert torch.equal(o1, o2) and torch.equal(f1, f2) and torch.equal(q1, q2)
    for n in g1:
        assert torch.equal(g1[n], g2[n]), n


def test_srlitmodule_five_adam_steps_and_strict_reload(dev, tmp_path):
    """Five Adam steps of SRLitModule(arch="diinn", mode=3, init_q=True) with the switches on, 12 x 10 -> 31 x 27: the loss is finite
    and decreases, every decoder tensor moved, and the weights reload with strict=True into a fresh module that evaluates to the
    trained module's output bit for bit."""
    import diinn_amd.modules as M
    torch.manual_seed(0)
    lit = M.SRLitModule(arch="diinn", mode=3, init_q=True).to(dev).train()
    for k, v in SWITCHES.items():
        setattr(lit.net.decoder, k, v)
    opt = torch.optim.Adam(lit.parameters(), lr=1e-4)
    lr = torch.rand(2, 3, 12, 10, device=dev)
    batch = {2.6: (lr, torch.rand(2, 3, 31, 27, device=dev), ["a", "b"])}
    before = {n: p.detach().clone() for n, p in lit.net.decoder.named_parameters()}
    assert len(before) == 20
    losses = []
    for _ in range(5):
        opt.zero_grad(set_to_none=True)
        loss, _ = lit.step(batch)
        loss.backward()
        for n, p in lit.net.decoder.named_parameters():
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n
        opt.step()
        losses.append(float(loss.detach()))
    print("losses", losses)
    assert all(np.isfinite(losses))
    assert losses[-1] < losses[0], losses
    for n, p in lit.net.decoder.named_parameters():
        assert not torch.equal(p.detach(), before[n]), n
    path = tmp_path / "initq_split_trained.ckpt"
    torch.save(lit.state_dict(), path)
    fresh = M.SRLitModule(arch="diinn", mode=3, init_q=True)
    fresh.load_state_dict(torch.load(path, map_location="cpu"), strict=True)
    fresh = fresh.to(dev).eval()
    for k, v in SWITCHES.items():
        setattr(fresh.net.decoder, k, v)
    lit.eval()
    with torch.no_grad():
        assert torch.equal(fresh(lr, (31, 27)), lit(lr, (31, 27)))
