"""Training path of the decoder with ``init_q=True`` and modes 1, 2 and 4, GPU part: ``ImplicitDecoder(mode, init_q=True,
hip_initq_modes=True, hip_autograd_initq_modes=True)`` under autograd on the HIP kernels against the REAL reference's fixtures;
``pixel_chain_bwd_kernel`` alone; the fused backward against the formula sheet on the same saved planes; structure checks;
``SRLitModule`` steps.  (CPU part, fixtures' loader and bounds: tests/test_initq_modes_training.py.)"""
import ctypes as C

import numpy as np
import pytest
import torch

import diinn_amd.synth as synth
from test_initq_modes_training import CASES, GRAD_RTOL, MODES, check_against_fixture, gold, inputs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def ptr(x):
    return C.c_void_p(x.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def decoder_for(mode, sd, dev, **kw):
    import diinn_amd.decoder as D
    dec = D.ImplicitDecoder(mode=mode, init_q=True, **kw)
    dec.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return dec.to(dev).train()


# ---------------------------------------------------------------------------
# autograd against the reference
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode,name", CASES)
def test_autograd_against_reference_fixtures(mode, name, dev):
    """Output within 1e-4 max(1, |ref|), every gradient within 1e-4 max|ref| of the real reference's (fp32) run."""
    sd, feat, r, (b, h, w, hu, wu) = inputs(mode, name)
    dec = decoder_for(mode, sd, dev, hip_initq_modes=True, hip_autograd_initq_modes=True)
    x = torch.from_numpy(feat).to(dev).requires_grad_(True)
    out = dec(x, (hu, wu))
    assert out.requires_grad and tuple(out.shape) == (b, 3, hu, wu)
    (out * torch.from_numpy(r).to(dev)).sum().backward()
    ref = gold(mode, name)["out"]
    err = float(np.abs(out.detach().cpu().numpy() - ref).max())
    print(f"mode {mode} {name} out: err {err:.3e} / max|ref| {float(np.abs(ref).max()):.3e}")
    assert err <= 1e-4 * max(1.0, float(np.abs(ref).max()))
    check_against_fixture(mode, name, x.grad.cpu().numpy(), {n: p.grad.cpu().numpy() for n, p in dec.named_parameters()})


# ---------------------------------------------------------------------------
# pixel_chain_bwd_kernel alone
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [143, 1])
def test_pixel_chain_bwd_kernel_alone(n, dev):
    """143 pixels: five plane tiles in two workgroups, the last workgroup holds one tile, and that tile is ragged; and a single
    pixel.  Random G (its padding columns NaN: they are not read as data), random k planes with both signs and exact zeros, random
    weights.  Against the float64 recurrence within 2e-5 max|ref| per layer (test_cell_chain_bwd_kernel_alone's bound); G_3, the
    rows 256..511 of every group, the padding columns and a guard band untouched (bit patterns); two runs bit-identical."""
    import diinn_amd._native as N
    import diinn_amd.initq_training as IT
    import diinn_amd.training as T
    lib = N.load()
    t = (n + 31) // 32
    if n == 143:
        assert t == 5 and n % 32 == 15
    sd = synth.decoder_state_dict(7, 1.0, mode=3, init_q=True)
    gen = torch.Generator().manual_seed(11)
    for i in (1, 2, 3):                                          # weights of order 1 / 16: every layer's product counts beside the term added
        sd[f"K.{i}.0.weight"] = (torch.randn((256, 832, 1, 1), generator=gen) / 16).numpy()
    p = {k: torch.from_numpy(v).to(dev) for k, v in sd.items()}
    packed = IT.pack_body_on_device(p)
    g_plain = torch.randn((4, 512, n), generator=gen)
    a_plain = torch.randn((4, 512, n), generator=gen)
    a_plain[:, :256][torch.rand((4, 256, n), generator=gen) < 0.25] = 0.0
    assert bool((a_plain[:, :256] == 0).any()) and bool((a_plain[:, :256] < 0).any()) and bool((a_plain[:, :256] > 0).any())
    guard, fill = 4096, -77.0
    g_buf = torch.full((4 * t * 512 * 32 + guard,), fill, device=dev)
    g_t = g_buf[:-guard].view(4, t, 512, 32)
    g_t.copy_(torch.stack([T.tile_planes(g_plain[i]) for i in range(4)]))
    acts = torch.stack([T.tile_planes(a_plain[i]) for i in range(4)]).to(dev)
    if n % 32:
        g_t[:, -1, :, n % 32:] = float("nan")
        acts[:, -1, :, n % 32:] = float("nan")
    before = g_buf.clone()
    second = g_buf.clone()
    assert lib.diinn_pixel_chain_bwd(stream(), ptr(g_buf), ptr(acts), ptr(packed), n) == 0
    assert lib.diinn_pixel_chain_bwd(stream(), ptr(second), ptr(acts), ptr(packed), n) == 0
    torch.cuda.synchronize()
    assert torch.equal(g_buf.view(torch.int32), second.view(torch.int32))
    b_t = before[:-guard].view(4, t, 512, 32)
    bits = lambda x: x.contiguous().view(torch.int32)             # noqa: E731
    assert torch.equal(bits(g_buf[-guard:]), bits(before[-guard:])), "guard band written"
    assert torch.equal(bits(g_t[3]), bits(b_t[3])), "G_3 written"
    assert torch.equal(bits(g_t[:, :, 256:]), bits(b_t[:, :, 256:])), "g_s rows written"
    if n % 32:
        assert torch.equal(bits(g_t[:, -1, :, n % 32:]), bits(b_t[:, -1, :, n % 32:])), "padding columns written"
    got = T.untile_planes(g_t, n).double()
    g64, k64 = g_plain.double().to(dev), a_plain[:, :256].double().to(dev)
    ga = g64[3, :256]
    for i in (3, 2, 1):
        kk = p[f"K.{i}.0.weight"].reshape(256, 832)[:, :256].double()
        ga = (k64[i - 1] > 0) * (kk.t() @ ga) + g64[i - 1, :256]
        err, top = float((got[i - 1, :256] - ga).abs().max()), float(ga.abs().max())
        print(f"n {n} g_a,{i - 1}: err {err:.3e} / max {top:.3e} = {err / top:.2e}")
        assert err <= 2e-5 * top, (i, err, top)
        assert float((got[i - 1, :256] - g64[i - 1, :256]).abs().max()) > 0.1 * top      # the layer's product is no rounding matter


# ---------------------------------------------------------------------------
# the fused backward against the formula sheet
# ---------------------------------------------------------------------------
_planes = {}


def forward_planes(mode, name, dev):
    """One training forward per (mode, case), shared by the tests below and left unchanged."""
    if (mode, name) not in _planes:
        import diinn_amd.initq_modes_training as MT
        import diinn_amd.training as T
        sd, feat, r, (b, h, w, hu, wu) = inputs(mode, name)
        params = [torch.from_numpy(sd[n]).to(dev) for n in MT.INITQ_PARAM_NAMES]
        f = torch.from_numpy(feat).to(dev)
        out, acts, packed, image, head = MT.train_forward_initq_modes(f, params, hu, wu, 2, mode)
        n = b * hu * wu
        plain = T.untile_planes(acts, n).reshape(4, 2, 256, n)
        _planes[(mode, name)] = (params, f, torch.from_numpy(r).to(dev), (hu, wu), out, acts, plain, packed, image, head)
    return _planes[(mode, name)]


@pytest.mark.parametrize("name", ["b2_12x10_31x27", "b1_8x8_5x6_down"])
@pytest.mark.parametrize("mode", MODES)
def test_fused_backward_against_the_formula_sheet_on_the_same_planes(mode, name, dev):
    """backward_fused_initq_modes against backward_from_saved_initq_modes in float64 on the planes the GPU forward saved: per tensor
    within 1e-4 max|ref|.  The saved planes and the output themselves: within 1e-4 of the float64 forward."""
    import diinn_amd.initq_modes_training as MT
    params, f, r, size, out, acts, plain, packed, image, head = forward_planes(mode, name, dev)
    p64 = [p.double() for p in params]
    out64, acts64 = MT.forward_planes_initq_modes(f.double(), p64, size, mode)
    assert float((out.double() - out64).abs().max()) <= 1e-4 * max(1.0, float(out64.abs().max()))
    assert float((plain.double() - acts64).abs().max()) <= 1e-4 * max(1.0, float(acts64.abs().max()))
    d_feat, d_params = MT.backward_fused_initq_modes(r, f, acts, packed, image, size, mode, head=head)
    w_feat, w_params = MT.backward_from_saved_initq_modes(r.double(), f.double(), plain.double(), p64, size, mode)
    bad = []
    for pname, got, want in [("feat", d_feat, w_feat)] + list(zip(MT.INITQ_PARAM_NAMES, d_params, w_params)):
        assert tuple(got.shape) == tuple(want.shape), pname
        err, top = float((got.double() - want).abs().max()), float(want.abs().max())
        print(f"mode {mode} {name} {pname}: err {err:.3e} / max {top:.3e} = {err / max(top, 1e-30):.2e}")
        if not err <= GRAD_RTOL * top:
            bad.append((pname, err, top))
    assert not bad, bad
    none_feat, _ = MT.backward_fused_initq_modes(r, f, acts, packed, image, size, mode, head=head, need_feat_grad=False)
    assert none_feat is None


# ---------------------------------------------------------------------------
# structure
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_two_passes_are_bit_identical(mode, dev):
    import diinn_amd.initq_modes_training as MT
    params, f, r, size, out, acts, plain, packed, image, head = forward_planes(mode, "b2_12x10_31x27", dev)
    f1, g1 = MT.backward_fused_initq_modes(r, f, acts, packed, image, size, mode, head=head)
    f2, g2 = MT.backward_fused_initq_modes(r, f, acts, packed, image, size, mode, head=head)
    assert torch.equal(f1, f2)
    for pname, a, b_ in zip(MT.INITQ_PARAM_NAMES, g1, g2):
        assert torch.equal(a, b_), pname
    out2, acts2, _, _, _ = MT.train_forward_initq_modes(f, params, size[0], size[1], 2, mode)
    assert torch.equal(out, out2)
    import diinn_amd.training as T
    n = f.shape[0] * size[0] * size[1]
    assert torch.equal(T.untile_planes(acts, n), T.untile_planes(acts2, n))


def test_mode1_is_mode2_with_zero_feature_columns(dev):
    """A mode-1 decoder and the mode-2 decoder whose K.1..3 are mode 1's widened by zero feature columns: the same output and the same
    gradients of every shared tensor, bit for bit (K.1..3: mode 2's [:, :256])."""
    import diinn_amd.initq_modes_training as MT
    sd, feat, r, (b, h, w, hu, wu) = inputs(1, "b2_12x10_31x27")
    sd2 = dict(sd)
    for i in (1, 2, 3):
        wide = np.zeros((256, 832, 1, 1), np.float32)
        wide[:, :256] = sd[f"K.{i}.0.weight"]
        sd2[f"K.{i}.0.weight"] = wide
    res = {}
    for mode, s in ((1, sd), (2, sd2)):
        dec = decoder_for(mode, s, dev, hip_initq_modes=True, hip_autograd_initq_modes=True)
        x = torch.from_numpy(feat).to(dev).requires_grad_(True)
        out = dec(x, (hu, wu))
        (out * torch.from_numpy(r).to(dev)).sum().backward()
        res[mode] = (out.detach(), x.grad, {n: p_.grad for n, p_ in dec.named_parameters()})
    assert torch.equal(res[1][0], res[2][0]) and torch.equal(res[1][1], res[2][1])
    for n in MT.INITQ_PARAM_NAMES:
        g1, g2 = res[1][2][n], res[2][2][n]
        if n in ("K.1.0.weight", "K.2.0.weight", "K.3.0.weight"):
            g2 = g2[:, :256]
        assert torch.equal(g1, g2), n
        assert float(g1.abs().max()) > 0, n


def test_mode4_with_a_centre_tap_head_is_mode3_with_init_q(dev):
    """Mode 4 whose 3x3 head has only its centre tap, carrying a mode-3 head L: the saved planes are those of mode 3 with init_q
    bit for bit, and so is every gradient but the head's own (bwd_head3x3_kernel's gates are bwd_head_kernel's term for term: the
    property test_mode4_training_gpu.py pins for init_q=False); the head's weight gradient has L's at the centre tap within 1e-5."""
    import diinn_amd.initq_modes_training as MT
    import diinn_amd.initq_training as IT
    import diinn_amd.training as T
    b, h, w, hu, wu = 3, 7, 5, 23, 18
    n = b * hu * wu
    sd3 = synth.decoder_state_dict(41, 1.0, mode=3, init_q=True)
    p3 = [torch.from_numpy(sd3[name]).to(dev) for name in IT.INITQ_PARAM_NAMES]
    li = IT.INITQ_PARAM_NAMES.index("last_layer.weight")
    lw4 = torch.zeros((3, 256, 3, 3), device=dev)
    lw4[:, :, 1, 1] = p3[li].view(3, 256)
    p4 = list(p3)
    p4[li] = lw4
    feat = torch.from_numpy(synth.encoder_features(41, b, h, w)).to(dev)
    r = torch.from_numpy(synth.uniform(41, "g", (b, 3, hu, wu), 1.0)).to(dev)
    out4, acts4, body4, image4, head4 = MT.train_forward_initq_modes(feat, p4, hu, wu, 2, 4)
    out3, acts3, body3, image3 = IT.train_forward_initq(feat, p3, hu, wu, 2)
    assert torch.equal(T.untile_planes(acts4, n), T.untile_planes(acts3, n))
    assert float((out4 - out3).abs().max()) <= 1e-5 * max(1.0, float(out3.abs().max()))     # two summation orders of 256 fp32 terms
    f4, g4 = MT.backward_fused_initq_modes(r, feat, acts4, body4, image4, (hu, wu), 4, head=head4)
    f3, g3 = IT.backward_fused_initq(r, feat, acts3, body3, image3, (hu, wu))
    assert torch.equal(f4, f3) and float(f3.abs().max()) > 0
    for name, a, b_ in zip(IT.INITQ_PARAM_NAMES, g4, g3):
        if name == "last_layer.weight":
            assert float((a[:, :, 1, 1] - b_.view(3, 256)).abs().max()) <= 1e-5 * float(b_.abs().max())
        else:
            assert torch.equal(a, b_), name


@pytest.mark.parametrize("mode", MODES)
def test_switch_leaves_the_no_grad_output_alone(mode, dev):
    """With the switch on, the no_grad output of the same decoder is bit-equal to its output with the switch off; with ``bsize`` given
    a call under grad is the no_grad inference path (no graph, the same bits); with the switch off the call under grad still
    raises.  The training forward's output (sines of radians, at the accurate sine as well) agrees with the inference output
    (revolutions) within the 1e-5 max(1, |out|) the mode-3 init_q training test holds that pair to -- not bit for bit, in any mode
    (mode 4's training forward has no such property without init_q either: test_mode4_training_gpu.py prints the distance)."""
    sd, feat, r, (b, h, w, hu, wu) = inputs(mode, "b2_12x10_31x27")
    for sin_mode in (2, 0):
        dec = decoder_for(mode, sd, dev, hip_initq_modes=True, sin_mode=sin_mode)
        x = torch.from_numpy(feat).to(dev)
        with pytest.raises(NotImplementedError, match="inference only"):
            dec(x, (hu, wu))
        with torch.no_grad():
            off = dec(x, (hu, wu))
        dec.hip_autograd_initq_modes = True
        with torch.no_grad():
            on = dec(x, (hu, wu))
        assert torch.equal(on, off)
        strips = dec(x, (hu, wu), 30000)
        assert not strips.requires_grad and torch.equal(strips, off)
        trained = dec(x, (hu, wu))
        assert trained.requires_grad
        dist = float((trained.detach() - off).abs().max())
        print(f"mode {mode} sin {sin_mode}: max|train out - no_grad out| = {dist:.3e}")
        assert dist <= 1e-5 * max(1.0, float(off.abs().max()))


# ---------------------------------------------------------------------------
# SRLitModule
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_srlitmodule_five_adam_steps_and_strict_reload(mode, dev, tmp_path):
    """Five Adam steps of SRLitModule(arch="diinn", mode=m, init_q=True) with the two switches on, a batch of 2 x 8 x 8 -> x3: the
    loss is finite and changes, every decoder tensor gets a finite gradient and moves, and the weights reload into a fresh module
    with strict=True, which then evaluates to the trained module's output bit for bit."""
    import diinn_amd.modules as M
    torch.manual_seed(0)
    lit = M.SRLitModule(arch="diinn", mode=mode, init_q=True).to(dev).train()
    lit.net.decoder.hip_initq_modes = True
    lit.net.decoder.hip_autograd_initq_modes = True
    opt = torch.optim.Adam(lit.parameters(), lr=1e-4)
    lr = torch.rand(2, 3, 8, 8, device=dev)
    batch = {3: (lr, torch.rand(2, 3, 24, 24, device=dev), ["a", "b"])}
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
    print("mode", mode, "losses", losses)
    assert all(np.isfinite(losses))
    assert len(set(losses)) == 5, losses
    for n, p in lit.net.decoder.named_parameters():
        assert not torch.equal(p.detach(), before[n]), n
    path = tmp_path / f"initq_m{mode}_trained.ckpt"
    torch.save(lit.state_dict(), path)
    fresh = M.SRLitModule(arch="diinn", mode=mode, init_q=True)
    fresh.load_state_dict(torch.load(path, map_location="cpu"), strict=True)
    fresh.net.decoder.hip_initq_modes = True
    fresh = fresh.to(dev).eval()
    lit.eval()
    with torch.no_grad():
        assert torch.equal(fresh(lr, (24, 24)), lit(lr, (24, 24)))
