"""Training path of the decoder with ``init_q=True``, mode 3, GPU part: ``ImplicitDecoder(mode=3, init_q=True, hip_autograd=True)``
under autograd on the HIP kernels against the REAL reference's fixtures; the fused backward against the formula sheet on the same
saved planes; ``initq_bwd_kernel``, the R-row cell sum and the fold alone; determinism; a NaN feature; ``SRLitModule`` steps; the
switch leaves inference alone.  (CPU part, fixtures' loader and bounds: tests/test_initq_training.py.)"""
import ctypes as C

import numpy as np
import pytest
import torch

import diinn_amd.synth as synth
from test_initq_training import CASE_NAMES, GRAD_RTOL, check_against_fixture, gold, inputs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch.device("cuda:0")


def decoder_for(sd, dev, **kw):
    import diinn_amd.decoder as D
    dec = D.ImplicitDecoder(mode=3, init_q=True, **kw)
    dec.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return dec.to(dev).train()


_runs = {}


def autograd_run(name, dev):
    """(out, d_feat, {name: grad}) of one autograd pass through the decoder with the switch on; computed once per case."""
    if name not in _runs:
        sd, feat, r, (b, h, w, hu, wu) = inputs(name)
        dec = decoder_for(sd, dev, hip_autograd=True)
        x = torch.from_numpy(feat).to(dev).requires_grad_(True)
        out = dec(x, (hu, wu))
        assert out.requires_grad and tuple(out.shape) == (b, 3, hu, wu)
        (out * torch.from_numpy(r).to(dev)).sum().backward()
        _runs[name] = (out.detach().cpu().numpy(), x.grad.cpu().numpy(), {n: p.grad.cpu().numpy() for n, p in dec.named_parameters()})
    return _runs[name]


@pytest.mark.parametrize("name", CASE_NAMES)
def test_autograd_against_reference_fixtures(name, dev):
    """Output within 1e-4 max(1, |ref|), every gradient within 1e-4 max|ref| of the real reference's (fp32) run."""
    out, d_feat, grads = autograd_run(name, dev)
    ref = gold(name)["out"]
    err = float(np.abs(out - ref).max())
    print(f"{name} out: err {err:.3e} / max|ref| {float(np.abs(ref).max()):.3e}")
    assert err <= 1e-4 * max(1.0, float(np.abs(ref).max()))
    check_against_fixture(name, d_feat, grads)


def _forward_planes(name, dev):
    import diinn_amd.initq_training as IT
    import diinn_amd.training as T
    sd, feat, r, (b, h, w, hu, wu) = inputs(name)
    params = [torch.from_numpy(sd[n]).to(dev) for n in IT.INITQ_PARAM_NAMES]
    f = torch.from_numpy(feat).to(dev)
    out, acts, packed, image = IT.train_forward_initq(f, params, hu, wu, 2)
    n = b * hu * wu
    plain = T.untile_planes(acts, n).reshape(4, 2, 256, n)
    return params, f, torch.from_numpy(r).to(dev), (hu, wu), out, acts, plain, packed, image


@pytest.mark.parametrize("name", ["b2_12x10_31x27", "b1_8x8_5x6_down", "b1_3x2_9x4"])
def test_fused_backward_against_the_formula_sheet_on_the_same_planes(name, dev):
    """backward_fused_initq against backward_from_saved_initq in float64 on the planes the GPU forward saved: per tensor within
    1e-4 max|ref|.  The saved planes themselves: within 1e-4 of the float64 forward."""
    import diinn_amd.initq_training as IT
    params, f, r, size, out, acts, plain, packed, image = _forward_planes(name, dev)
    d_feat, d_params = IT.backward_fused_initq(r, f, acts, packed, image, size)
    w_feat, w_params = IT.backward_from_saved_initq(r.double(), f.double(), plain.double(), [p.double() for p in params], size)
    bad = []
    for pname, got, want in [("feat", d_feat, w_feat)] + list(zip(IT.INITQ_PARAM_NAMES, d_params, w_params)):
        assert tuple(got.shape) == tuple(want.shape), pname
        err, top = float((got.double() - want).abs().max()), float(want.abs().max())
        print(f"{name} {pname}: err {err:.3e} / max {top:.3e} = {err / max(top, 1e-30):.2e}")
        if not err <= GRAD_RTOL * top:
            bad.append((pname, err, top))
    assert not bad, bad
    none_feat, _ = IT.backward_fused_initq(r, f, acts, packed, image, size, need_feat_grad=False)
    assert none_feat is None


def test_initq_bwd_kernel_alone(dev):
    """1 x 5 x 6 -> 13 x 11 = 143 pixels: five plane tiles in three workgroups, the last workgroup with one tile, that tile ragged.
    Random G (its padding columns NaN: they are not read as data); U, da, x', E against float64 tensor algebra to 1e-5 max; the
    padding rows 576..639 of x' and E exactly zero; the padding columns of the last tile and a guard band behind every buffer
    untouched."""
    import diinn_amd._native as N
    import diinn_amd.initq_training as IT
    import diinn_amd.training as T
    lib = N.load()
    b, h, w, hu, wu = 1, 5, 6, 13, 11
    n = b * hu * wu
    t = (n + 31) // 32
    assert t == 5 and n % 32 == 15
    sd = synth.decoder_state_dict(123, 1.0, mode=3, init_q=True)
    image = IT.pack_initq_train(sd).to(dev)
    feat = torch.from_numpy(synth.encoder_features(123, b, h, w)).to(dev)
    gen = torch.Generator().manual_seed(5)
    g_plain = torch.randn((4, 512, n), generator=gen)
    g_t = torch.stack([T.tile_planes(g_plain[i]) for i in range(4)]).to(dev)
    g_t[:, -1, :, n % 32:] = float("nan")
    guard, fill = 4096, -77.0
    sizes = {"u": 576, "da": 576, "xp": 640, "e": 640}
    bufs = {k: torch.full((t * rows * 32 + guard,), fill, device=dev) for k, rows in sizes.items()}
    ptr = lambda x: C.c_void_p(x.data_ptr())                      # noqa: E731
    st = lib.diinn_initq_backward(C.c_void_p(torch.cuda.current_stream().cuda_stream), ptr(feat), ptr(g_t), ptr(image),
                                  ptr(bufs["u"]), ptr(bufs["da"]), ptr(bufs["xp"]), ptr(bufs["e"]), b, h, w, hu, wu)
    assert st == 0
    torch.cuda.synchronize()
    # float64 tensor algebra
    p64 = {k: torch.from_numpy(v).double().to(dev) for k, v in sd.items()}
    a, xc, _ = IT.embedding_planes(feat.double(), p64, (hu, wu))
    e, cos_a = torch.sin(a), torch.cos(a)
    g64 = g_plain.double().to(dev)
    wx = [p64["K.0.0.weight"].reshape(256, 576)] + [p64[f"K.{i}.0.weight"].reshape(256, 832)[:, 256:] for i in (1, 2, 3)]
    dxp = sum(wx[i].t() @ g64[i, :256] for i in range(4))
    want = {"u": dxp * e, "da": (dxp * xc + p64["Q.0.0.weight"].reshape(256, 576).t() @ g64[0, 256:]) * cos_a, "xp": e * xc, "e": e}
    for k, rows in sizes.items():
        assert bool((bufs[k][-guard:] == fill).all()), f"{k}: guard band written"
        tiled = bufs[k][:-guard].view(t, rows, 32)
        assert bool((tiled[-1, :, n % 32:] == fill).all()), f"{k}: padding columns of the ragged tile written"
        got = T.untile_planes(tiled, n)
        if rows == 640:
            assert bool((got[576:] == 0).all()), f"{k}: padding rows are not exactly zero"
        err, top = float((got[:576].double() - want[k]).abs().max()), float(want[k].abs().max())
        print(f"{k}: err {err:.3e} / max {top:.3e} = {err / top:.2e}")
        assert err <= 1e-5 * top, (k, err, top)


@pytest.mark.parametrize("shape", [(2, 3, 2, 7, 5), (1, 1, 1, 7, 5), (1, 8, 8, 5, 6), (1, 6, 4, 24, 16)])
def test_fold_and_cell_sum_alone(shape, dev):
    """diinn_cell_sum_rows (R = 576 rows of one tiled group -> NCHW, zeros for a cell that owns no pixel) against an index-add and
    diinn_fold3x3 against F.fold, both in float64: this test calls torch as the oracle, the product path does not."""
    import diinn_amd._native as N
    import diinn_amd.training as T
    lib = N.load()
    b, h, w, hu, wu = shape
    n = b * hu * wu
    gen = torch.Generator().manual_seed(3)
    u = torch.randn((576, n), generator=gen).to(dev)
    u_t = T.tile_planes(u)
    if n % 32:
        u_t[-1, :, n % 32:] = float("nan")                        # the padding is not read
    geo = T._geometry(b, h, w, hu, wu, dev)
    idx_h, _, idx_w, _, _ = T.coordinate_tensors(h, w, hu, wu, dev)
    guard = 1024
    big = torch.full((b * 576 * h * w + guard,), float("nan"), device=dev)
    ptr = lambda x: C.c_void_p(x.data_ptr())                      # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.diinn_cell_sum_rows(stream, ptr(u_t), 576, 576, ptr(geo["seg_h"]), ptr(geo["seg_w"]), ptr(big), b, h, w, hu, wu) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(big[-guard:]).all())
    d_unf = big[:-guard].view(b, 576, h, w)
    cell = (idx_h[:, None] * w + idx_w[None, :]).reshape(-1)                                  # [Hu*Wu] -> cy * W + cx
    want = torch.zeros((b, 576, h * w), dtype=torch.float64, device=dev)
    want.index_add_(2, cell, u.double().view(576, b, hu * wu).permute(1, 0, 2).contiguous())
    err = float((d_unf.double().view(b, 576, h * w) - want).abs().max())
    assert err <= 1e-5 * float(want.abs().max()), err
    owned = torch.zeros(h * w, dtype=torch.bool, device=dev)
    owned[cell] = True
    assert bool((d_unf.view(b, 576, h * w)[:, :, ~owned] == 0).all())                          # exactly zero where no pixel lands
    if shape == (1, 8, 8, 5, 6):
        assert int((~owned).sum()) >= 30
    bigf = torch.full((b * 64 * h * w + guard,), float("nan"), device=dev)
    assert lib.diinn_fold3x3(stream, ptr(d_unf), ptr(bigf), b, 64, h, w) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(bigf[-guard:]).all())
    wantf = torch.nn.functional.fold(d_unf.double().reshape(b, 576, h * w), (h, w), 3, padding=1)
    errf = float((bigf[:-guard].view(b, 64, h, w).double() - wantf).abs().max())
    assert errf <= 1e-5 * max(float(wantf.abs().max()), 1e-30), errf


def test_two_backward_passes_are_bit_identical(dev):
    import diinn_amd.initq_training as IT
    params, f, r, size, out, acts, plain, packed, image = _forward_planes("b2_12x10_31x27", dev)
    f1, g1 = IT.backward_fused_initq(r, f, acts, packed, image, size)
    f2, g2 = IT.backward_fused_initq(r, f, acts, packed, image, size)
    assert torch.equal(f1, f2)
    for pname, a, b_ in zip(IT.INITQ_PARAM_NAMES, g1, g2):
        assert torch.equal(a, b_), pname
    # and the forward: the same planes, the same output
    out2, acts2, _, _ = IT.train_forward_initq(f, params, size[0], size[1], 2)
    assert torch.equal(out, out2)
    n = f.shape[0] * size[0] * size[1]
    import diinn_amd.training as T
    assert torch.equal(T.untile_planes(acts, n), T.untile_planes(acts2, n))


def test_the_two_init_q_images_are_not_interchangeable(dev):
    """The inference kernels answer NaN on the training image (radians) and the training forward answers NaN on the inference image
    (revolutions): each form of initq_planes_kernel accepts its own validity word only."""
    import diinn_amd._native as N
    import diinn_amd.decoder as D
    import diinn_amd.initq_training as IT
    sd, feat, r, (b, h, w, hu, wu) = inputs("b1_3x2_9x4")
    f = torch.from_numpy(feat).to(dev)
    body = D.pack_state_dict(D.initq_body_state_dict(sd), mode=3).to(dev)
    train_image, infer_image = IT.pack_initq_train(sd).to(dev), D.pack_initq(sd).to(dev)
    assert bool(torch.isfinite(D.decode_features(f, body, (hu, wu), initq=infer_image)).all())
    assert bool(torch.isnan(D.decode_features(f, body, (hu, wu), initq=train_image)).all())
    params = [torch.from_numpy(sd[n]).to(dev) for n in IT.INITQ_PARAM_NAMES]
    out, acts, packed, image = IT.train_forward_initq(f, params, hu, wu, 2)
    assert bool(torch.isfinite(out).all()) and torch.equal(image.cpu().view(torch.int32), train_image.cpu().view(torch.int32))
    lib = N.load()
    pix = torch.empty(lib.diinn_initq_pix_bytes(b, wu, hu) // 4, device=dev)
    out2, acts2 = torch.empty_like(out), torch.empty_like(acts)
    ptr = lambda x: C.c_void_p(x.data_ptr())                      # noqa: E731
    st = lib.diinn_decode_initq_train_fwd(C.c_void_p(torch.cuda.current_stream().cuda_stream), ptr(f), ptr(packed), ptr(infer_image), ptr(pix),
                                          ptr(out2), ptr(acts2), b, h, w, hu, wu, 2)
    assert st == 0
    assert bool(torch.isnan(out2).all())


def test_a_nan_feature_stays_in_its_neighbourhood(dev):
    """One NaN in feat (batch item 0, cell (6, 4) of 12 x 10): the output is NaN at exactly the pixels of the 3 x 3 cells that read it;
    d feat may be NaN only at cells whose 3 x 3 neighbourhood holds the NaN, and every cell whose 3 x 3 neighbourhood holds none of
    those nine cells -- everything outside the 5 x 5 box, and all of batch item 1 -- keeps the bits of the clean run."""
    import diinn_amd.initq_training as IT
    import diinn_amd.training as T
    name = "b2_12x10_31x27"
    sd, feat, r, (b, h, w, hu, wu) = inputs(name)
    params = [torch.from_numpy(sd[n]).to(dev) for n in IT.INITQ_PARAM_NAMES]
    rr = torch.from_numpy(r).to(dev)
    res = []
    for poison in (False, True):
        f = torch.from_numpy(feat).to(dev)
        if poison:
            f[0, 5, 6, 4] = float("nan")
        out, acts, packed, image = IT.train_forward_initq(f, params, hu, wu, 2)
        d_feat, _ = IT.backward_fused_initq(rr, f, acts, packed, image, (hu, wu))
        res.append((out, d_feat))
    (out0, df0), (out1, df1) = res
    idx_h, _, idx_w, _, _ = T.coordinate_tensors(h, w, hu, wu, dev)
    near_h, near_w = (idx_h - 6).abs() <= 1, (idx_w - 4).abs() <= 1
    hit = torch.zeros((b, hu, wu), dtype=torch.bool, device=dev)
    hit[0] = near_h[:, None] & near_w[None, :]
    assert bool(torch.isnan(out1).all(1)[hit].all()) and torch.equal(out1.permute(0, 2, 3, 1)[~hit], out0.permute(0, 2, 3, 1)[~hit])
    box3 = torch.zeros((b, h, w), dtype=torch.bool, device=dev)
    box3[0, 5:8, 3:6] = True
    box5 = torch.zeros((b, h, w), dtype=torch.bool, device=dev)
    box5[0, 4:9, 2:7] = True
    nan_cells = torch.isnan(df1).any(1)
    assert not bool((nan_cells & ~box3).any())
    assert torch.equal(df1.permute(0, 2, 3, 1)[~box5], df0.permute(0, 2, 3, 1)[~box5])
    assert bool(torch.isfinite(df0).all())


def test_srlitmodule_five_adam_steps_and_strict_reload(dev, tmp_path):
    """Five Adam steps of SRLitModule(arch="diinn", mode=3, init_q=True) with the switch on, a batch of 2 x 12 x 12 -> x2: the loss is
    finite and decreases, every decoder tensor moved, and the weights reload into a fresh module with strict=True, which then
    evaluates to the trained module's output bit for bit."""
    import diinn_amd.modules as M
    torch.manual_seed(0)
    lit = M.SRLitModule(arch="diinn", mode=3, init_q=True).to(dev).train()
    lit.net.decoder.hip_autograd = True
    opt = torch.optim.Adam(lit.parameters(), lr=1e-4)
    lr = torch.rand(2, 3, 12, 12, device=dev)
    batch = {2: (lr, torch.rand(2, 3, 24, 24, device=dev), ["a", "b"])}
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
    path = tmp_path / "initq_trained.ckpt"
    torch.save(lit.state_dict(), path)
    fresh = M.SRLitModule(arch="diinn", mode=3, init_q=True)
    fresh.load_state_dict(torch.load(path, map_location="cpu"), strict=True)
    fresh = fresh.to(dev).eval()
    lit.eval()
    with torch.no_grad():
        assert torch.equal(fresh(lr, (24, 24)), lit(lr, (24, 24)))


def test_switch_leaves_the_no_grad_output_alone(dev):
    """With the switch on, the no_grad output of the same decoder is bit-equal to its output with the switch off; with ``bsize`` given
    a call under grad is the no_grad inference path (no graph, the same bits); with the switch off the call under grad still raises."""
    sd, feat, r, (b, h, w, hu, wu) = inputs("b2_12x10_31x27")
    dec = decoder_for(sd, dev)
    x = torch.from_numpy(feat).to(dev)
    with pytest.raises(NotImplementedError, match="autograd"):
        dec(x, (hu, wu))
    with torch.no_grad():
        off = dec(x, (hu, wu))
    dec.hip_autograd = True
    with torch.no_grad():
        on = dec(x, (hu, wu))
    assert torch.equal(on, off)
    strips = dec(x, (hu, wu), 30000)
    assert not strips.requires_grad and torch.equal(strips, off)
    trained = dec(x, (hu, wu))
    assert trained.requires_grad
    assert float((trained.detach() - off).abs().max()) <= 1e-5 * max(1.0, float(off.abs().max()))
