"""Training path of decoder mode 4, GPU part: head3x3_taps_from_planes_kernel and bwd_head3x3_kernel alone, the centre-tap identity
with mode 3's backward, ``ImplicitDecoder(mode=4, hip_autograd_mode4=True)`` under autograd against the REAL reference's fixtures,
determinism, ``SRLitModule`` steps.  (CPU part, the fixtures' loader and bounds: tests/test_mode4_training.py.)"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import diinn_amd.synth as synth
from test_mode4_training import CASE_NAMES, check_against_fixture, gold, inputs

pytestmark = pytest.mark.gpu

ptr = lambda x: C.c_void_p(x.data_ptr())                          # noqa: E731
same = lambda x, y: bool(((x == y) | (torch.isnan(x) & torch.isnan(y))).all())   # noqa: E731


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def body_word_image(word, dev):
    """A body image of which only the validity word exists (the two head kernels of the forward read nothing else of it)."""
    import diinn_amd.training as T
    at = T._section(6)[0] + 3
    img = torch.zeros(at + 1, dtype=torch.float32, device=dev)
    img[at:].view(torch.int32).fill_(word)
    return img


# ---------------------------------------------------------------------------
# 6. kernel 1 alone
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 23, 18), (1, 2, 2)])
def test_taps_from_planes_kernel_alone(dev, shape):
    """Random k_3, s_3 planes (the other groups and the last tile's padding NaN: never read as data) -> taps and out against a float64
    torch computation within 1e-5 max|ref| (the plane-kernel tests' bound); float 27 of every pixel zero; nothing written behind the
    tap buffer; a head image without its word, or a body image with neither word, answers NaN; both body words are accepted."""
    import diinn_amd._native as N
    import diinn_amd.decoder as D
    import diinn_amd.training as T
    lib = N.load()
    b, hu, wu = shape
    n = b * hu * wu
    t = (n + 31) // 32
    if b == 3:
        assert n == 1242 and n % 32 == 26 and t == 39
    sd = synth.decoder_state_dict(11, 1.0, mode=4)
    head = D.pack_head3x3(sd).to(dev)
    gen = torch.Generator().manual_seed(n)
    k3 = torch.relu(torch.randn((256, n), generator=gen))
    s3 = 3.0 * torch.randn((256, n), generator=gen)
    acts = torch.full((4, t, 512, 32), float("nan"), device=dev)
    acts[3] = T.tile_planes(torch.cat([k3, s3], 0)).to(dev)
    if n % 32:
        acts[3, -1, :, n % 32:] = float("nan")
    guard, fill = 1024, -77.0
    taps = torch.full((n * 28 + guard,), fill, device=dev)
    out = torch.full((b, 3, hu, wu), fill, device=dev)
    body = body_word_image(N.PACKED_MAGIC_WPU, dev)
    assert lib.diinn_head3x3_from_planes(stream(), ptr(acts), ptr(body), ptr(head), ptr(taps), ptr(out), b, hu, wu) == 0
    torch.cuda.synchronize()
    q64 = (k3.double() * torch.sin(s3.double()))
    lw, lb = torch.from_numpy(sd["last_layer.weight"]).double(), torch.from_numpy(sd["last_layer.bias"]).double()
    want_taps = (lw.permute(2, 3, 0, 1).reshape(27, 256) @ q64).t()                          # [n, 27]
    want_out = F.conv2d(F.pad(q64.view(256, b, hu, wu).permute(1, 0, 2, 3), (1, 1, 1, 1), mode="reflect"), lw, lb)
    got = taps[:n * 28].view(n, 28).cpu()
    err_t = float((got[:, :27].double() - want_taps).abs().max())
    err_o = float((out.cpu().double() - want_out).abs().max())
    print(f"{shape}: taps err {err_t:.3e} / max {float(want_taps.abs().max()):.3e}; out err {err_o:.3e} / max {float(want_out.abs().max()):.3e}")
    assert err_t <= 1e-5 * float(want_taps.abs().max())
    assert err_o <= 1e-5 * float(want_out.abs().max())
    assert not bool(got[:, 27].any())
    assert bool((taps[n * 28:] == fill).all())
    # validity words
    out2 = torch.empty_like(out)
    assert lib.diinn_head3x3_from_planes(stream(), ptr(acts), ptr(body_word_image(N.PACKED_MAGIC, dev)), ptr(head), ptr(taps), ptr(out2),
                                         b, hu, wu) == 0
    assert torch.equal(out2, out)
    bad_head = head.clone()
    bad_head[-1] = 0.0
    assert lib.diinn_head3x3_from_planes(stream(), ptr(acts), ptr(body), ptr(bad_head), ptr(taps), ptr(out2), b, hu, wu) == 0
    assert bool(torch.isnan(out2).all()) and bool(torch.isnan(taps[:n * 28].view(n, 28)[:, :27]).all())
    assert lib.diinn_head3x3_from_planes(stream(), ptr(acts), ptr(body_word_image(0, dev)), ptr(head), ptr(taps), ptr(out2), b, hu, wu) == 0
    assert bool(torch.isnan(out2).all())


# ---------------------------------------------------------------------------
# 7. kernel 3 alone
# ---------------------------------------------------------------------------
_planes = {}


def cpu_planes(name):
    """(params, feat, R, (b, hu, wu), acts [4,2,256,N]) of a fixture case, the planes from the torch restatement; once per case."""
    import diinn_amd.mode4_training as M4
    import diinn_amd.training as T
    if name not in _planes:
        sd, feat, r, (b, h, w, hu, wu) = inputs(name)
        params = [torch.from_numpy(sd[n]) for n in T.PARAM_NAMES]
        with torch.no_grad():
            _, acts = M4.forward_torch_mode4(torch.from_numpy(feat), params, (hu, wu))
        _planes[name] = (params, torch.from_numpy(feat), torch.from_numpy(r), (b, hu, wu), acts)
    return _planes[name]


@pytest.mark.parametrize("name", ["c1x1_2x2", "row3x2_2x7", "col4x3_9x2", "b3_7x5_23x18"])
def test_bwd_head3x3_kernel_alone(dev, name):
    """diinn_backward_data_head3x3 on the restatement's planes: G_3, q_3 and the seven dT groups against the formula sheet in
    float64 within 5e-5 of each plane's scale (the bound of test_fused_backward_equals_formula_backward_on_gpu); row 27 of dT zero;
    the padding of a ragged last tile untouched in G, Q and dT; the layers below finite."""
    import diinn_amd._native as N
    import diinn_amd.decoder as D
    import diinn_amd.mode4_training as M4
    import diinn_amd.training as T
    lib = N.load()
    params, feat, r, (b, hu, wu), acts = cpu_planes(name)
    n = b * hu * wu
    t = (n + 31) // 32
    pd = [p_.to(dev) for p_ in params]
    body, head = M4.images_on_device(pd)
    assert np.array_equal(head.cpu().numpy().view(np.uint32),
                          D.pack_head3x3({"last_layer.weight": params[16].numpy(), "last_layer.bias": params[17].numpy()}).numpy().view(np.uint32))
    acts_t = torch.stack([T.tile_planes(acts[i].reshape(512, n)) for i in range(4)]).to(dev)
    if n % 32:
        acts_t[:, -1, :, n % 32:] = float("nan")
    gp = r.permute(1, 0, 2, 3).reshape(3, n).contiguous().to(dev)
    fill = -77.0
    g_t = torch.full((4, t, 512, 32), float("nan"), device=dev)
    q_t = torch.full((4, t, 256, 32), float("nan"), device=dev)
    dt_t = torch.full((7, t, 4, 32), fill, device=dev)
    assert lib.diinn_backward_data_head3x3(stream(), ptr(gp), ptr(acts_t), ptr(body), ptr(head), ptr(g_t), ptr(q_t), ptr(dt_t),
                                           b, hu, wu) == 0
    torch.cuda.synchronize()
    a64 = acts.double()
    d_t = M4.head_adjoint_taps(r.double()).permute(1, 0, 2, 3).reshape(27, n)
    hrows = params[16].double().permute(2, 3, 0, 1).reshape(27, 256)
    g_q = hrows.t() @ d_t
    ga = g_q * torch.sin(a64[3, 1]) * (a64[3, 0] > 0)
    gs = g_q * a64[3, 0] * torch.cos(a64[3, 1])
    q3 = a64[3, 0] * torch.sin(a64[3, 1])
    g = T.untile_planes(g_t, n).view(4, 2, 256, n).cpu()
    q = T.untile_planes(q_t, n).cpu()
    got_dt = T.untile_planes(dt_t, n).reshape(28, n).cpu()
    scale = max(float(ga.abs().max()), float(gs.abs().max()), 1e-12)
    errs = (float((g[3, 0].double() - ga).abs().max()), float((g[3, 1].double() - gs).abs().max()),
            float((q[3].double() - q3).abs().max()), float((got_dt[:27].double() - d_t).abs().max()))
    print(f"{name}: g_a,3 {errs[0]:.3e} g_s,3 {errs[1]:.3e} (scale {scale:.3e}); q_3 {errs[2]:.3e} (max {float(q3.abs().max()):.3e}); "
          f"dT {errs[3]:.3e} (max {float(d_t.abs().max()):.3e})")
    assert errs[0] <= 5e-5 * scale and errs[1] <= 5e-5 * scale
    assert errs[2] <= 5e-5 * max(1.0, float(q3.abs().max()))
    assert errs[3] <= 5e-5 * float(d_t.abs().max())
    assert not bool(got_dt[27].any())
    assert torch.isfinite(g).all() and torch.isfinite(q).all()
    if n % 32:
        assert torch.isnan(g_t.permute(0, 2, 1, 3).reshape(4, 512, -1)[..., n:]).all()
        assert torch.isnan(q_t.permute(0, 2, 1, 3).reshape(4, 256, -1)[..., n:]).all()
        assert bool((dt_t[:, -1, :, n % 32:] == fill).all())


# ---------------------------------------------------------------------------
# 8. the centre-tap identity
# ---------------------------------------------------------------------------
def test_centre_tap_head_is_mode3_backward_bit_for_bit(dev):
    """A 3x3 head whose only non-zero tap is k = 4, carrying a mode-3 head L: dT[12..14] = g and every other term of the FMA chain
    is 0 * x, so G and Q of diinn_backward_data_head3x3 are bit-identical to diinn_backward_data on the mode-3 image with head L
    (which computes g_q,3 = L^T g in the same three-term order) -- all four layers, padding included."""
    import diinn_amd._native as N
    import diinn_amd.mode4_training as M4
    import diinn_amd.training as T
    lib = N.load()
    b, h, w, hu, wu = 3, 7, 5, 23, 18
    n = b * hu * wu
    t = (n + 31) // 32
    sd3 = synth.decoder_state_dict(41, 1.0, mode=3)
    p3 = [torch.from_numpy(sd3[name]).to(dev) for name in T.PARAM_NAMES]
    lw4 = torch.zeros((3, 256, 3, 3), device=dev)
    lw4[:, :, 1, 1] = p3[16].view(3, 256)
    p4 = [*p3[:16], lw4, p3[17]]
    feat = torch.from_numpy(synth.encoder_features(41, b, h, w)).to(dev)
    out, acts, body, head = M4.train_forward_mode4(feat, p4, hu, wu, 2)
    gp = torch.from_numpy(synth.uniform(41, "g", (3, n), 1.0)).to(dev)
    g4 = torch.full((4, t, 512, 32), float("nan"), device=dev)
    q4 = torch.full((4, t, 256, 32), float("nan"), device=dev)
    dt_t = torch.zeros((7, t, 4, 32), device=dev)
    assert lib.diinn_backward_data_head3x3(stream(), ptr(gp), ptr(acts), ptr(body), ptr(head), ptr(g4), ptr(q4), ptr(dt_t), b, hu, wu) == 0
    packed3 = T.pack_on_device(p3)
    g3 = torch.full((4, t, 512, 32), float("nan"), device=dev)
    q3 = torch.full((4, t, 256, 32), float("nan"), device=dev)
    assert lib.diinn_backward_data(stream(), ptr(gp), ptr(acts), ptr(packed3), ptr(g3), ptr(q3), n) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(T.untile_planes(g3, n)).all() and float(T.untile_planes(g3, n).abs().max()) > 0
    assert same(g4, g3) and same(q4, q3)
    # and the forward: with that head mode 4's training output is mode 3's on the same planes, up to the two heads' summation orders
    # (256 fp32 terms each: the plane-kernel tests' 1e-5 of the scale)
    out3 = T.DecodeMode3Function.apply(feat, hu, wu, 2, *p3)
    assert float((out - out3).abs().max()) <= 1e-5 * max(1.0, float(out3.abs().max()))


# ---------------------------------------------------------------------------
# 9. end to end, 10. determinism
# ---------------------------------------------------------------------------
def decoder_for(sd, dev, **kw):
    import diinn_amd.decoder as D
    dec = D.ImplicitDecoder(mode=4, **kw)
    dec.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return dec.to(dev).train()


def autograd_run(name, dev, sin_mode):
    sd, feat, r, (b, h, w, hu, wu) = inputs(name)
    dec = decoder_for(sd, dev, hip_autograd_mode4=True, sin_mode=sin_mode)
    x = torch.from_numpy(feat).to(dev).requires_grad_(True)
    out = dec(x, (hu, wu))
    assert out.requires_grad and tuple(out.shape) == (b, 3, hu, wu)
    (out * torch.from_numpy(r).to(dev)).sum().backward()
    with torch.no_grad():
        infer = dec(x.detach(), (hu, wu))
    return out.detach(), infer, x.grad, {n: p.grad for n, p in dec.named_parameters()}


@pytest.mark.parametrize("sin_mode", [0, 1, 2])
@pytest.mark.parametrize("name", CASE_NAMES)
def test_autograd_against_reference_fixtures(name, sin_mode, dev):
    """Output within 1e-4 max(1, |ref|), every gradient within 1e-4 max|ref| of the real reference's (fp32) run, in every sine mode.
    Printed, without a bound of its own: the distance between the training forward's out and the no_grad mode-4 out."""
    out, infer, d_feat, grads = autograd_run(name, dev, sin_mode)
    ref = gold(name)["out"]
    err = float(np.abs(out.cpu().numpy() - ref).max())
    print(f"{name} sin {sin_mode} out: err {err:.3e} / max|ref| {float(np.abs(ref).max()):.3e}; "
          f"max|train out - no_grad out| = {float((out - infer).abs().max()):.3e}")
    assert err <= 1e-4 * max(1.0, float(np.abs(ref).max()))
    check_against_fixture(name, d_feat.cpu().numpy(), {n: g.cpu().numpy() for n, g in grads.items()})


def test_two_backward_passes_are_bit_identical(dev):
    a = autograd_run("b3_7x5_23x18", dev, 2)
    b_ = autograd_run("b3_7x5_23x18", dev, 2)
    assert torch.equal(a[0], b_[0]) and torch.equal(a[2], b_[2])
    for n in a[3]:
        assert torch.equal(a[3][n], b_[3][n]), n


# ---------------------------------------------------------------------------
# 11. optimiser steps
# ---------------------------------------------------------------------------
def test_training_step_decreases_loss_and_needs_the_switch(dev):
    """A few Adam steps of SRLitModule.step (sr_module.py:113-125,127-129) on one synthetic batch with the switch on: the L1 loss goes
    down, i.e. encoder, decoder and 3x3 head gradients flow through the HIP path.  With the switch off the same call raises."""
    import diinn_amd.modules as M
    torch.manual_seed(0)
    net = M.SRLitModule(arch="diinn", mode=4, init_q=False).to(dev).train()
    lr = torch.rand(2, 3, 16, 16, device=dev)
    batch = {2: (lr, torch.rand(2, 3, 32, 32, device=dev), ["a", "b"]),
             3: (lr, torch.rand(2, 3, 48, 48, device=dev), ["a", "b"])}
    with pytest.raises(NotImplementedError, match="hip_autograd_mode4"):
        net.step(batch)
    net.net.decoder.hip_autograd_mode4 = True
    opt = torch.optim.Adam(net.parameters(), lr=1e-4)
    head0 = net.net.decoder.last_layer.weight.detach().clone()
    losses = []
    for _ in range(6):
        opt.zero_grad(set_to_none=True)
        loss, _ = net.step(batch)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert all(np.isfinite(losses))
    assert losses[-1] < losses[0], losses
    assert not torch.equal(net.net.decoder.last_layer.weight.detach(), head0)
