"""LIIF under autograd in split-bf16 arithmetic on the GPU (``LIIF.hip_autograd_split_bf16``): liif_x3_save_kernel
(``diinn_liif_train_fwd_x3``) and liif_bwd_layer_x3_kernel (``diinn_liif_backward_data_x3``) against the float64 oracle and the
emulation sheet, always with PINNED gates -- the float64 side of a gradient comparison runs on the kernel's own planes, upcast --
the mixed forms, the module against the real reference's fixtures, determinism, the cache, ``SRLitModule`` and the C ABI.

Shapes, inputs and CPU-side sheets: tests/test_liif_split_training.py.  The reference is always float64, the fp32 path or a fixture,
never the code under test."""
import ctypes as C

import numpy as np
import pytest
import torch

import test_liif_split_training as S
import test_liif_training as TL

pytestmark = pytest.mark.gpu

PNAMES, RTOL, ATOL = S.PNAMES, S.RTOL, S.ATOL


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return torch.device("cuda:0")


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _host_images(ws, dev):
    """(packed, split) from the host packers: what inference decodes with (the packed image carries the validity word)."""
    import diinn_amd.decoder as D
    host = D.pack_liif_state_dict({"imnet." + n: x for n, x in zip(PNAMES, ws)})
    return host.to(dev), D.pack_liif_split(host).to(dev)


def _planes(acts, b, hu, wu):
    """Tiled [4 layers][T][256][32] -> h_1..h_4, each [4 members, N, 256]."""
    import diinn_amd.liif_training as LT
    saved = LT.saved_activations(acts, b, hu, wu)                 # [4 members][4 layers][256][N]
    return [saved[:, l].permute(0, 2, 1).contiguous() for l in range(4)]


def _untile(g, n):
    """One tiled group [T][256][32] over the virtual pixels -> [4 members, N, 256]."""
    import diinn_amd.training as T
    return T.untile_planes(g, 4 * n).reshape(256, 4, n).permute(1, 2, 0).contiguous()


def _padding_is_nan(group, n):
    """The padding of a ragged last tile of every layer of ``group`` [L][T][256][32] is still the NaN it was filled with."""
    return (4 * n) % 32 == 0 or bool(torch.isnan(group[:, -1, :, (4 * n) % 32:]).all())


def _split_forward(name, dev, grad=False):
    """The split training forward through the Python path on the device-gathered images: (params, feat, image, split, out, acts)."""
    import diinn_amd.liif_split_training as LS
    import diinn_amd.liif_training as LT
    ws, feat, _r, (b, h, w, hu, wu) = S.case(name)
    params = [torch.from_numpy(x).to(dev).requires_grad_(grad) for x in ws]
    f = torch.from_numpy(feat).to(dev)
    image, split = LT.image_on_device(params), LS.split_on_device(params)
    out, acts = LS.train_forward_split(f.contiguous(), image, split, hu, wu)
    return params, f, image, split, out, acts


def _fused(name, dev, params, f, acts, image, split):
    import diinn_amd.liif_training as LT
    _ws, _feat, r, (b, h, w, hu, wu) = S.case(name)
    p0 = params[0]
    return LT.backward_fused(torch.from_numpy(r).to(dev), f, acts, image, p0.detach(), ("liif", p0.data_ptr(), p0._version), (p0,),
                             (hu, wu), split=split)


@pytest.mark.parametrize("name", S.ALL)
def test_forward_planes_and_output(name, dev):
    """``diinn_liif_train_fwd_x3`` through the C ABI on NaN-filled buffers: ``out`` is ``diinn_liif_decode_x3``'s bit for bit; ``h_1`` is
    ``diinn_liif_train_fwd``'s bit for bit (layer 1 is fp32 in both); ``h_2..h_4`` are within 1e-4 x max(1, max|a_64|) of float64 and of
    the sheet; every element below 4 N is finite and the padding of a ragged last tile is still NaN; the gates of layers 2..4 differ
    from float64's within the CPU test's caps.
    Measured (MI355X): |hip - f64| at most 7.2e-5 against 9.9e-4 (gain3 h_4; the sheet: 7.3e-5), 5.4e-6 against 1.1e-4 at gain 1;
    |hip - sheet| at most 4.4e-5; gates that differ on b2_12x10_31x27: 2 + 6 + 3 = 11 (cap 52; the sheet: 12), 0 on the other nine."""
    import diinn_amd._native as N
    import diinn_amd.decoder as D
    import diinn_amd.liif_training as LT
    lib = N.load()
    ws, feat, _r, (b, h, w, hu, wu) = S.case(name)
    n = b * hu * wu
    packed, split = _host_images(ws, dev)
    f = torch.from_numpy(feat).to(dev).contiguous()
    t = LT.virtual_tiles(n)
    out = torch.full((b, 3, hu, wu), float("nan"), device=dev)
    acts = torch.full((4, t, 256, 32), float("nan"), device=dev)
    acts32 = torch.full((4, t, 256, 32), float("nan"), device=dev)
    out32 = torch.empty((b, 3, hu, wu), device=dev)
    wk = torch.empty(lib.diinn_workspace_bytes(b, h, w) // 4, device=dev)
    want = D.liif_decode_features(f, packed, (hu, wu), split=split)
    torch.cuda.synchronize()
    assert lib.diinn_liif_train_fwd_x3(_stream(), _ptr(f), _ptr(packed), _ptr(split), _ptr(wk), _ptr(out), _ptr(acts), b, h, w, hu, wu) == 0
    assert lib.diinn_liif_train_fwd(_stream(), _ptr(f), _ptr(packed), _ptr(wk), _ptr(out32), _ptr(acts32), b, h, w, hu, wu) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, want)
    hs, hs32 = _planes(acts, b, hu, wu), _planes(acts32, b, hu, wu)
    assert torch.equal(hs[0], hs32[0])
    assert all(bool(torch.isfinite(x).all()) for x in hs) and _padding_is_nan(acts, n)
    a_x3, a_64 = S.sheets(name)
    differ = 0
    for l in range(4):
        got = hs[l].cpu().double()
        e64 = float((got - torch.relu(a_64[l])).abs().max())
        esh = float((got - torch.relu(a_x3[l]).double()).abs().max())
        s64 = float((torch.relu(a_x3[l]).double() - torch.relu(a_64[l])).abs().max())
        bound = ATOL * max(1.0, float(a_64[l].abs().max()))
        d = int(((hs[l].cpu() > 0) != (a_64[l] > 0)).sum())
        print(f"liif split fwd {name} h_{l + 1}: |hip - f64| {e64:.3e}  |hip - sheet| {esh:.3e}  |sheet - f64| {s64:.3e}  (bound {bound:.3e}), "
              f"{d} gates differ from float64")
        assert e64 <= bound and esh <= bound, (name, l, e64, esh, bound)
        differ += d if l else 0
    assert differ <= S.gate_cap(name, n), (name, differ)


@pytest.mark.parametrize("name", S.ALL)
def test_backward_with_pinned_gates(name, dev):
    """The test of liif_bwd_layer_x3_kernel; the ReLU kink cannot disturb it.  The kernel's own planes, upcast, go through float64
    ``liif_backward_from_saved``: d feat and the ten parameter gradients of ``backward_fused(..., split=)`` are within
    1e-4 x max|ref| per tensor.  A direct ``diinn_liif_backward_data_x3`` call on NaN-filled ``G``: the planes G[0..3] are within
    1e-4 x max|ref| of the float64 chain on those planes, G[3] is ``diinn_liif_backward_data``'s G[3] bit for bit on the same acts, the
    ragged padding is not written.  The kernel's and the sheet's distances are printed side by side.
    Measured (MI355X): planes and gradients at most 9.2e-6 x max|f64| on the ten shapes, level with the sheet.
    (A dropped product costs about 2^-9 relative, more than 10x the bound: checked once in a scratch build with w_hi.g_lo dropped --
    G[2] 1.9e-3 x max|f64| off on 9x4 and on b2_12x10_31x27, this test fails -- see DESIGN.md 3.8.)"""
    import diinn_amd._native as N
    import diinn_amd.liif_split_training as LS
    lib = N.load()
    _ws, _feat, r, (b, h, w, hu, wu) = S.case(name)
    n = b * hu * wu
    params, f, image, split, _out, acts = _split_forward(name, dev)
    rr = torch.from_numpy(r).to(dev)
    hs = _planes(acts, b, hu, wu)
    h64, p64 = [x.double() for x in hs], [p.detach().double() for p in params]
    c64 = LS.liif_split_chain_reference(rr.double(), h64, p64, (h, w), split=False)
    csh = LS.liif_split_chain_reference(rr, hs, [p.detach() for p in params], (h, w))
    # the chain alone, through the C ABI
    gp = rr.permute(1, 0, 2, 3).reshape(3, n).contiguous()
    G = torch.full_like(acts, float("nan"))
    G32 = torch.full_like(acts, float("nan"))
    torch.cuda.synchronize()
    assert lib.diinn_liif_backward_data_x3(_stream(), _ptr(gp), _ptr(acts), _ptr(image), _ptr(split), _ptr(G), b, h, w, hu, wu) == 0
    assert lib.diinn_liif_backward_data(_stream(), _ptr(gp), _ptr(acts), _ptr(image), _ptr(G32), b, h, w, hu, wu) == 0
    torch.cuda.synchronize()
    assert _padding_is_nan(G, n)
    assert torch.equal(_untile(G[3], n), _untile(G32[3], n))
    for i in range(4):                                            # c64[i] = g_a,(4 - i) = slot 3 - i
        got = _untile(G[3 - i], n)
        assert bool(torch.isfinite(got).all())
        err, ers, scale = float((got.double() - c64[i]).abs().max()), float((csh[i].double() - c64[i]).abs().max()), float(c64[i].abs().max())
        e32 = float((_untile(G32[3 - i], n).double() - c64[i]).abs().max())
        print(f"liif split bwd {name} G[{3 - i}]: kernel {err:.3e}  sheet {ers:.3e}  fp32 kernel {e32:.3e}  max|f64| {scale:.3e} (bound {RTOL * scale:.3e})")
        assert err <= RTOL * scale, (name, 3 - i, err, scale)
    # the whole backward
    d64, g64 = LS.liif_backward_from_saved(rr.double(), f.double(), h64, p64, (hu, wu))
    dsh, gsh = LS.liif_backward_from_saved(rr, f, hs, [p.detach() for p in params], (hu, wu), chain=csh)
    d_feat, grads = _fused(name, dev, params, f, acts, image, split)
    for pname, got, sh, ref in zip(["feat"] + PNAMES, [d_feat] + grads, [dsh] + gsh, [d64] + g64):
        err, ers, scale = float((got.double() - ref).abs().max()), float((sh.double() - ref).abs().max()), float(ref.abs().max())
        print(f"liif split bwd {name} {pname}: kernel {err:.3e}  sheet {ers:.3e}  max|f64| {scale:.3e} (bound {RTOL * scale:.3e})")
        assert err <= RTOL * scale, (name, pname, err, scale)


@pytest.mark.parametrize("name", S.ALL)
def test_mixed_forms(name, dev):
    """The planes keep the fp32 contract: the split forward's planes through the fp32 ``diinn_liif_backward_data`` (the bisecting
    tool) against the split backward on the same planes, <= 1e-4 relative per tensor; and the fp32 forward's planes through the
    split backward against the fp32 backward on those."""
    import diinn_amd.liif_training as LT
    _ws, _feat, _r, (b, h, w, hu, wu) = S.case(name)
    params, f, image, split, _out, acts = _split_forward(name, dev)
    _o32, acts32 = LT.train_forward(f.contiguous(), image, hu, wu)
    for tag, a in (("split fwd", acts), ("fp32 fwd", acts32)):
        d_s, g_s = _fused(name, dev, params, f, a, image, split)
        d_f, g_f = _fused(name, dev, params, f, a, image, None)
        for pname, x, ref in zip(["feat"] + PNAMES, [d_s] + g_s, [d_f] + g_f):
            err, scale = float((x.double() - ref.double()).abs().max()), float(ref.abs().max())
            print(f"liif split mixed {name} {tag} {pname}: |x3 bwd - fp32 bwd| {err:.3e} = {err / max(scale, 1e-30):.2e} max|fp32|")
            assert err <= RTOL * scale, (name, tag, pname, err, scale)


def test_end_to_end_against_the_real_reference(dev):
    """``LIIF(hip_autograd=True, hip_split_bf16=True, hip_autograd_split_bf16=True)`` on given features, the five fixtures of the real
    reference (as tests/test_liif_training.py::test_liif_autograd_against_reference_fixtures): ``y`` under grad is the no_grad output
    of the same module bit for bit; with ``bsize`` the output carries no graph and is equal; every gradient is within 1e-4 x max|ref|
    of the fixture's .grad.  A case is compared only if its saved planes show no gate that differs from float64's (the kink is not
    the kernels' to hold); at most one of the five may drop out that way -- by the sheet none does.
    Measured (MI355X): none drops out; worst gradient 1.2e-5 x max|ref| (layers.0.weight of b2_3x2_5x4)."""
    dropped = []
    for name in S.FIXTURES:
        ws, feat, r, (b, h, w, hu, wu) = S.case(name)
        net = TL._model(ws, dev, hip_autograd=True, hip_split_bf16=True, hip_autograd_split_bf16=True)
        x = torch.from_numpy(feat).to(dev).requires_grad_(True)
        net.encoder = TL._GivenFeatures(x)
        inp = torch.zeros((b, 3, h, w), device=dev)
        y = net(inp, (hu, wu))
        assert y.requires_grad
        with torch.no_grad():
            y0 = net(inp, (hu, wu))
        assert torch.equal(y.detach(), y0)
        yb = net(inp, (hu, wu), 300)
        assert not yb.requires_grad and torch.equal(yb, y0)
        ref_out = TL.gold(name)["out"]
        assert float(np.abs(y0.cpu().numpy() - ref_out).max()) <= ATOL * max(1.0, float(np.abs(ref_out).max()))
        (y * torch.from_numpy(r).to(dev)).sum().backward()
        _p, _f, _i, _s, out, acts = _split_forward(name, dev)
        assert torch.equal(out, y0)                                   # the planes looked at are this forward's
        a_64 = S.sheets(name)[1]
        differ = sum(int(((hl.cpu() > 0) != (a > 0)).sum()) for hl, a in zip(_planes(acts, b, hu, wu), a_64))
        if differ:
            print(f"liif split e2e {name}: DROPPED, {differ} gates differ from float64's")
            dropped.append(name)
            continue
        named = dict(net.imnet.named_parameters())
        TL._check_against_fixture(name, x.grad.cpu().numpy(), [named[p].grad.cpu().numpy() for p in PNAMES], RTOL, "hip split")
    assert len(dropped) <= 1, dropped


def test_determinism_needs_input_grad_and_cache(dev):
    """Two backward runs are bit-equal; ``feat`` without grad gives no d feat and frozen parameters no gradient, the rest the full
    run's values; after an in-place change of one imnet weight the next step equals a fresh module's (the split image is rebuilt
    per weight version)."""
    import diinn_amd.liif_split_training as LS
    ws, feat, r, (b, h, w, hu, wu) = S.case("b1_4x3_9x7")
    rr = torch.from_numpy(r).to(dev)

    def run(arrays, feat_grad, which):
        params = [torch.from_numpy(x).to(dev).requires_grad_(p in which) for p, x in zip(PNAMES, arrays)]
        x = torch.from_numpy(feat).to(dev).requires_grad_(feat_grad)
        y = LS.LIIFSplitFunction.apply(x, hu, wu, *params)
        (y * rr).sum().backward()
        return y.detach(), x.grad, [p.grad for p in params]

    y1, f1, g1 = run(ws, True, PNAMES)
    y2, f2, g2 = run(ws, True, PNAMES)
    assert torch.equal(y1, y2) and torch.equal(f1, f2) and all(torch.equal(a, c) for a, c in zip(g1, g2))
    _, f3, g3 = run(ws, False, ["layers.0.bias", "layers.4.weight"])
    assert f3 is None
    for i, p in enumerate(PNAMES):
        if p in ("layers.0.bias", "layers.4.weight"):
            assert torch.equal(g3[i], g1[i]), p
        else:
            assert g3[i] is None, p
    # the cache: one module, a step, an in-place change of a hidden weight, another step
    net = TL._model(ws, dev, hip_autograd=True, hip_split_bf16=True, hip_autograd_split_bf16=True)
    x = torch.from_numpy(feat).to(dev).requires_grad_(True)
    net.encoder = TL._GivenFeatures(x)
    inp = torch.zeros((b, 3, h, w), device=dev)
    (net(inp, (hu, wu)) * rr).sum().backward()
    assert torch.equal(x.grad, f1) and torch.equal(net.imnet.layers[4].weight.grad, g1[PNAMES.index("layers.4.weight")])
    with torch.no_grad():
        net.imnet.layers[4].weight.mul_(1.25)
    net.zero_grad(set_to_none=True)
    x.grad = None
    y = net(inp, (hu, wu))
    (y * rr).sum().backward()
    changed = [a.copy() for a in ws]
    changed[PNAMES.index("layers.4.weight")] = net.imnet.layers[4].weight.detach().cpu().numpy()
    yf, ff, gf = run(changed, True, PNAMES)
    assert not torch.equal(yf, y1)
    assert torch.equal(y.detach(), yf) and torch.equal(x.grad, ff)
    named = dict(net.imnet.named_parameters())
    assert all(torch.equal(named[p].grad, g) for p, g in zip(PNAMES, gf))


def test_srlitmodule_trains_with_the_three_switches(dev):
    """``SRLitModule(arch="liif")`` with the three lines set: six Adam steps on B = 2 of 16 x 16 at x2 and x3 decrease the loss.  With
    the new line missing, ``step`` raises the "trains in fp32 only" text."""
    import diinn_amd.modules as M
    torch.manual_seed(0)
    net = M.SRLitModule(arch="liif").to(dev).train()
    net.net.hip_autograd = True
    net.net.hip_split_bf16 = True
    lr = torch.rand(2, 3, 16, 16, device=dev)
    batch = {2: (lr, torch.rand(2, 3, 32, 32, device=dev), ["a", "b"]),
             3: (lr, torch.rand(2, 3, 48, 48, device=dev), ["a", "b"])}
    with pytest.raises(NotImplementedError, match="LIIF trains in fp32 only"):
        net.step(batch)
    net.net.hip_autograd_split_bf16 = True
    opt = torch.optim.Adam(net.parameters(), lr=1e-4)
    losses = []
    for _ in range(6):
        opt.zero_grad(set_to_none=True)
        loss, _ = net.step(batch)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    print("liif split SRLitModule losses:", " ".join(f"{v:.5f}" for v in losses))
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses


def test_c_abi_refusals(dev):
    """Null pointers, bad dims and a misaligned ``split_dev`` answer what the fp32 entry points answer for the same faults; every case
    returns before the first launch (the NaN-filled outputs stay NaN).  No bad pointer that would be dereferenced is sent."""
    import diinn_amd._native as N
    lib = N.load()
    ws, feat, r, (b, h, w, hu, wu) = S.case("b1_4x3_9x7")
    n = b * hu * wu
    params, f, image, split, _out, acts = _split_forward("b1_4x3_9x7", dev)
    out = torch.full((b, 3, hu, wu), float("nan"), device=dev)
    A = torch.full_like(acts, float("nan"))
    G = torch.full_like(acts, float("nan"))
    wk = torch.empty(lib.diinn_workspace_bytes(b, h, w) // 4, device=dev)
    gp = torch.from_numpy(r).to(dev).permute(1, 0, 2, 3).reshape(3, n).contiguous()
    INV, BIG = N.ERR_INVALID_ARG, N.ERR_TOO_LARGE
    st = _stream()
    fp, ip, sp, kp, op, ap = _ptr(f), _ptr(image), _ptr(split), _ptr(wk), _ptr(out), _ptr(A)
    good = (b, h, w, hu, wu)
    dims = [((0, h, w, hu, wu), INV), ((b, -1, w, hu, wu), INV), ((b, h, 0, hu, wu), INV), ((b, h, w, 0, wu), INV),
            ((b, h, w, hu, -3), INV), ((65536, h, w, hu, wu), BIG), ((b, 65536, w, hu, wu), BIG), ((b, h, w, 50000, 50000), BIG),
            ((1, h, w, 40000, 40000), BIG)]                          # 6.4e9 virtual pixels: past the training limit
    fwd = [((None, ip, sp, kp, op, ap), good, INV), ((fp, None, sp, kp, op, ap), good, INV), ((fp, ip, None, kp, op, ap), good, INV),
           ((fp, ip, sp, None, op, ap), good, INV), ((fp, ip, sp, kp, None, ap), good, INV), ((fp, ip, sp, kp, op, None), good, INV),
           ((None, ip, sp, kp, op, ap), (0, h, w, hu, wu), INV)] + [((fp, ip, sp, kp, op, ap), d, s) for d, s in dims]
    for (a_f, a_i, a_s, a_k, a_o, a_a), d, status in fwd:
        got = lib.diinn_liif_train_fwd_x3(st, a_f, a_i, a_s, a_k, a_o, a_a, *d)
        assert got == status, ("fwd", d, got, status)
        if a_s is not None:
            assert lib.diinn_liif_train_fwd(st, a_f, a_i, a_k, a_o, a_a, *d) == status, ("fp32 fwd", d)
    gpp, acp, Gp = _ptr(gp), _ptr(acts), _ptr(G)
    misaligned = C.c_void_p(split.data_ptr() + 4)
    bwd = [((None, acp, ip, sp, Gp), good, INV), ((gpp, None, ip, sp, Gp), good, INV), ((gpp, acp, None, sp, Gp), good, INV),
           ((gpp, acp, ip, None, Gp), good, INV), ((gpp, acp, ip, sp, None), good, INV),
           ((gpp, acp, ip, misaligned, Gp), good, INV)] + [((gpp, acp, ip, sp, Gp), d, s) for d, s in dims]
    for (a_g, a_c, a_i, a_s, a_G), d, status in bwd:
        got = lib.diinn_liif_backward_data_x3(st, a_g, a_c, a_i, a_s, a_G, *d)
        assert got == status, ("bwd", d, got, status)
        if a_s is not None and a_s is not misaligned:
            assert lib.diinn_liif_backward_data(st, a_g, a_c, a_i, a_G, *d) == status, ("fp32 bwd", d)
    # the fp32 entry's answer to a misaligned weight image is the same status
    assert lib.diinn_liif_backward_data(st, gpp, acp, C.c_void_p(image.data_ptr() + 4), Gp, *good) == INV
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(A).all()) and bool(torch.isnan(G).all())
