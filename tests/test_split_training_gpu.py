"""Mode 3 under autograd in split-bf16 arithmetic (ImplicitDecoder.hip_autograd_split_bf16): the GPU half.

decode_bf16x3_kernel<SAVE> (diinn_decode_train_fwd_x3), bwd_layer_x3_kernel (diinn_backward_data_x3) and the device packer of the
split training image, at the two fixture cases and five small shapes: one pixel (every tile ragged), ragged tiles in one and two
workgroups, a downscale, and N = 384 (whole tiles and whole workgroups only).

Every gradient comparison is either continuous or has the ReLU gates PINNED (the float64 formulas run on the kernel's own planes):
a pre-activation within the split rounding of zero lands on the other side of the kink, where the gate's gradient is discontinuous.
The end-to-end test (4) therefore compares a case only if its planes show no gate that differs from the oracle's."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import diinn_amd.synth as synth
import diinn_oracle as orc

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
HID = 256
ROW_STRIDE = 8
FIXTURES = {"grad_b2_12x10_31x27": (2, 12, 10, 31, 27, 1.0), "grad_b1_9x14_36x56_stress": (1, 9, 14, 36, 56, 3.0)}
SMALL = {"px1": (1, 1, 1, 1, 1, 1.0), "7x5": (1, 1, 1, 7, 5, 1.0), "9x4": (1, 3, 2, 9, 4, 1.0), "down_5x6": (1, 8, 8, 5, 6, 1.0),
         "n384": (1, 5, 7, 16, 24, 1.0)}
SHAPES = {**FIXTURES, **SMALL}
_cache = {}


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _case(name):
    """Inputs, oracle planes and the split forward's result through the C ABI on NaN-filled planes: computed once per shape."""
    if name in _cache:
        return _cache[name]
    import diinn_amd._native as N
    import diinn_amd.split_training as S
    import diinn_amd.training as T
    dev = torch.device("cuda:0")
    lib = N.load()
    b, h, w, hu, wu, gain = SHAPES[name]
    sd = synth.decoder_state_dict(123, gain)
    feat = synth.encoder_features(123, b, h, w)
    r = synth.uniform(123, f"gradw:{name}", (b, 3, hu, wu), 1.0)
    ref_out, ref_acts = orc.saved_planes(sd, feat, (hu, wu))
    params = [torch.from_numpy(sd[n_]).to(dev) for n_ in T.PARAM_NAMES]
    packed = T.pack_on_device(params).clone()
    split = S.pack_split_on_device(params).clone()
    f = torch.from_numpy(feat).to(dev)
    n = b * hu * wu
    t = (n + 31) // 32
    ws = torch.empty(b * h * w * 1024, device=dev)
    acts = torch.full((4, t, 512, 32), float("nan"), device=dev)
    out = torch.empty((b, 3, hu, wu), device=dev)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    N.check(lib.diinn_precompute_P_wpu(stream, _ptr(f), _ptr(packed), _ptr(ws), b, h, w, 0, h), "P")
    N.check(lib.diinn_decode_train_fwd_x3(stream, _ptr(ws), _ptr(packed), _ptr(split), _ptr(out), _ptr(acts), b, h, w, hu, wu,
                                          N.SIN_DEFAULT), "diinn_decode_train_fwd_x3")
    torch.cuda.synchronize()
    a = T.untile_planes(acts, n).view(4, 2, HID, n)
    flips = int(((a[1:, 0].cpu() > 0) != (ref_acts[1:, 0] > 0)).sum())
    _cache[name] = dict(sd=sd, feat=feat, r=r, ref_out=ref_out, ref_acts=ref_acts, params=params, packed=packed, split=split, f=f,
                        gout=torch.from_numpy(r).to(dev), out=out, acts=acts, planes=a, flips=flips, n=n, t=t, size=(hu, wu), dims=(b, h, w))
    return _cache[name]


def _rel(got, ref):
    return float((got.double() - ref.double()).abs().max()) / max(float(ref.abs().max()), 1e-6)


@pytest.mark.parametrize("name", list(SHAPES))
def test_forward_planes_and_output(name):
    """1. diinn_decode_train_fwd_x3 on NaN-filled planes: out and planes within 1e-4 * max(1, max|ref|) of orc.saved_planes, every
    element below N finite, a ragged last tile's padding still NaN, gates that differ from the oracle's at most 1e-5 of the
    3 * 256 * N split-layer elements (rounded up to at least 1)."""
    c = _case(name)
    n = c["n"]
    e_out = float((c["out"].cpu() - c["ref_out"]).abs().max()) / max(1.0, float(c["ref_out"].abs().max()))
    a = c["planes"].cpu()
    assert torch.isfinite(a).all()
    e_pl = float((a - c["ref_acts"]).abs().max()) / max(1.0, float(c["ref_acts"].abs().max()))
    print(f"{name}: out err {e_out:.2e}, planes err {e_pl:.2e}, gates that differ {c['flips']} of {3 * HID * n}")
    assert e_out <= 1e-4 and e_pl <= 1e-4
    flat = c["acts"].permute(0, 2, 1, 3).reshape(4, 512, -1)
    assert torch.isnan(flat[..., n:]).all()                # padding of the last tile is never written
    assert c["flips"] <= max(1, math.ceil(1e-5 * 3 * HID * n))


def _chain_planes64(c):
    """G_i = (g_a,i ; g_s,i) and q_i in float64 from the kernel's own planes (training.backward_from_saved's formulas)."""
    import diinn_amd.training as T
    a = c["planes"].double()
    p = {k: v.double() for k, v in zip(T.PARAM_NAMES, c["params"])}
    n = c["n"]
    g_q = p["last_layer.weight"].reshape(3, HID).t() @ c["gout"].double().permute(1, 0, 2, 3).reshape(3, n)
    gs, qs = [None] * 4, [None] * 4
    for i in (3, 2, 1, 0):
        k, s = a[i, 0], a[i, 1]
        g_a, g_s = g_q * torch.sin(s) * (k > 0), g_q * k * torch.cos(s)
        gs[i], qs[i] = torch.cat([g_a, g_s]), k * torch.sin(s)
        if i:
            g_q = p[f"K.{i}.0.weight"].reshape(HID, -1)[:, :HID].t() @ g_a + p[f"Q.{i}.0.weight"].reshape(HID, HID).t() @ g_s
    return gs, qs


@pytest.mark.parametrize("name", list(SHAPES))
def test_backward_with_pinned_gates(name):
    """2. The kernel's own planes, upcast, through float64 backward_from_saved: d feat and all 18 parameter gradients of
    backward_fused with the split chain within 1e-4 relative per tensor; the planes G_i, q_i of diinn_backward_data_x3 within
    1e-4 * max|ref| of the same formulas.  The test of bwd_layer_x3_kernel: the kink cannot disturb it."""
    import diinn_amd._native as N
    import diinn_amd.training as T
    c = _case(name)
    dev = c["f"].device
    n, t = c["n"], c["t"]
    d_feat, d_params = T.backward_fused(c["gout"], c["f"], c["acts"], c["params"], c["packed"], c["size"], split=c["split"])
    torch.cuda.synchronize()
    d_feat64, d_params64 = T.backward_from_saved(c["gout"], c["f"], c["planes"].double(), c["params"], c["size"])
    worst = ("feat", _rel(d_feat, d_feat64))
    for nm, got, ref in zip(T.PARAM_NAMES, d_params, d_params64):
        assert tuple(got.shape) == tuple(T.PARAM_SHAPES[nm])
        e = _rel(got, ref)
        if e > worst[1]:
            worst = (nm, e)
    g = torch.full((4, t, 512, 32), float("nan"), device=dev)
    q = torch.full((4, t, HID, 32), float("nan"), device=dev)
    gp = c["gout"].permute(1, 0, 2, 3).reshape(3, n).contiguous()
    N.check(N.load().diinn_backward_data_x3(C.c_void_p(torch.cuda.current_stream().cuda_stream), _ptr(gp), _ptr(c["acts"]), _ptr(c["packed"]),
                                            _ptr(c["split"]), _ptr(g), _ptr(q), n), "diinn_backward_data_x3")
    torch.cuda.synchronize()
    gs, qs = _chain_planes64(c)
    e_g = e_q = 0.0
    for i in range(4):
        gi, qi = T.untile_planes(g[i], n), T.untile_planes(q[i], n)
        assert torch.isfinite(gi).all() and torch.isfinite(qi).all()
        e_g = max(e_g, float((gi.double() - gs[i]).abs().max()) / max(float(gs[i].abs().max()), 1e-30))
        e_q = max(e_q, float((qi.double() - qs[i]).abs().max()) / max(float(qs[i].abs().max()), 1e-30))
    assert torch.isnan(g.permute(0, 2, 1, 3).reshape(4, 512, -1)[..., n:]).all()      # a ragged tile's padding is not written
    assert torch.isnan(q.permute(0, 2, 1, 3).reshape(4, HID, -1)[..., n:]).all()
    print(f"{name}: worst pinned gradient {worst[0]} {worst[1]:.2e}, planes G {e_g:.2e}, q {e_q:.2e}")
    assert worst[1] <= 1e-4, worst
    assert e_g <= 1e-4 and e_q <= 1e-4


@pytest.mark.parametrize("name", list(SHAPES))
def test_mixed_form_split_forward_under_the_fp32_backward(name):
    """3. The split forward's planes through the existing fp32 diinn_backward_data against the split backward on the same planes:
    within 1e-4 relative per tensor.  When 2 fails this tells which kernel is wrong."""
    import diinn_amd.training as T
    c = _case(name)
    f32 = T.backward_fused(c["gout"], c["f"], c["acts"], c["params"], c["packed"], c["size"])
    x3 = T.backward_fused(c["gout"], c["f"], c["acts"], c["params"], c["packed"], c["size"], split=c["split"])
    torch.cuda.synchronize()
    worst = ("feat", _rel(x3[0], f32[0]))
    for nm, got, ref in zip(T.PARAM_NAMES, x3[1], f32[1]):
        e = _rel(got, ref)
        if e > worst[1]:
            worst = (nm, e)
    print(f"{name}: split backward against the fp32 backward on the same planes: worst {worst[0]} {worst[1]:.2e}")
    assert worst[1] <= 1e-4, worst


def test_end_to_end_through_the_decoder():
    """4. ImplicitDecoder(mode=3, compute="bf16x3", hip_autograd_split_bf16=True): forward + .backward() against the real reference's
    fixtures (grad_b2_12x10_31x27) and the float64 oracle (the small gain-1 shapes) at 1e-4 relative.  A case is compared only if
    its kernel planes show no gate that differs from the oracle's (measured: down_5x6 has one such gate of 23,040 and drops out);
    at most one case may drop out that way.  On the parent this test fails with NotImplementedError."""
    import diinn_amd.decoder as D
    dev = torch.device("cuda:0")
    gold = np.load(os.path.join(HERE, "golden", "diinn_golden_grad.npz"))
    names = ["grad_b2_12x10_31x27", *SMALL]
    dropped = [nm for nm in names if _case(nm)["flips"]]
    assert len(dropped) <= 1, dropped
    for nm in names:
        if nm in dropped:
            continue
        c = _case(nm)
        hu, wu = c["size"]
        dec = D.ImplicitDecoder(mode=3, init_q=False, compute="bf16x3", hip_autograd_split_bf16=True)
        dec.load_state_dict({k: torch.from_numpy(v) for k, v in c["sd"].items()}, strict=True)
        dec = dec.to(dev).train()
        x = torch.from_numpy(c["feat"]).to(dev).requires_grad_(True)
        y = dec(x, [hu, wu])
        (y * c["gout"]).sum().backward()
        torch.cuda.synchronize()
        assert torch.equal(y.detach(), c["out"])              # the Function runs the kernel test 1 checked
        grads = {n_: p.grad.cpu() for n_, p in dec.named_parameters()}
        if nm in FIXTURES:
            ref = gold[f"grad/{nm}/feat"]
            worst = ("feat", float(np.abs(x.grad.cpu().numpy() - ref).max()) / float(np.abs(ref).max()))
            for pn, g in grads.items():
                ref = gold[f"grad/{nm}/{pn}"]
                g = g.numpy()[::ROW_STRIDE] if pn.startswith("K.") and pn.endswith("weight") else g.numpy()
                assert g.shape == ref.shape, (pn, g.shape, ref.shape)
                e = float(np.abs(g - ref).max()) / max(float(np.abs(ref).max()), 1e-6)
                if e > worst[1]:
                    worst = (pn, e)
        else:
            _, d_feat64, g64 = orc.reference_gradients(c["sd"], c["feat"], (hu, wu), c["r"], dtype=torch.float64)
            worst = ("feat", _rel(x.grad.cpu(), d_feat64))
            for pn, g in grads.items():
                e = _rel(g, g64[pn])
                if e > worst[1]:
                    worst = (pn, e)
        print(f"{nm}: end to end, worst gradient {worst[0]} {worst[1]:.2e}")
        assert worst[1] <= 1e-4, (nm, worst)


def test_training_step_decreases_loss_with_both_lines_set():
    """5. Six Adam steps of SRLitModule.step with lit.net.set_split_bf16() and lit.net.decoder.hip_autograd_split_bf16 = True on the
    two-scale synthetic batch of test_training_step_decreases_loss: finite and decreasing loss.  With the first line alone the step
    refuses, as on the parent."""
    import diinn_amd.modules as M
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    net = M.SRLitModule(arch="diinn", mode=3, init_q=False).to(dev).train()
    lr = torch.rand(2, 3, 16, 16, device=dev)
    batch = {2: (lr, torch.rand(2, 3, 32, 32, device=dev), ["a", "b"]),
             3: (lr, torch.rand(2, 3, 48, 48, device=dev), ["a", "b"])}
    net.net.set_split_bf16()
    with pytest.raises(NotImplementedError, match="autograd through the HIP decode path"):
        net.step(batch)
    net.net.decoder.hip_autograd_split_bf16 = True
    opt = torch.optim.Adam(net.parameters(), lr=1e-4)
    losses = []
    for _ in range(6):
        opt.zero_grad(set_to_none=True)
        loss, _ = net.step(batch)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert all(np.isfinite(losses))
    assert losses[-1] < losses[0], losses


def test_device_packer_is_the_host_twin_and_follows_the_weights():
    """6. The device packer's image equals the host twin's bit for bit (from the same gathered image); after an in-place optimiser
    step the parameter versions move and the cached split image is rebuilt."""
    import diinn_amd.split_training as S
    import diinn_amd.training as T
    dev = torch.device("cuda:0")
    sd = synth.decoder_state_dict(7, 1.0)
    params = [torch.nn.Parameter(torch.from_numpy(sd[n_]).to(dev)) for n_ in T.PARAM_NAMES]
    split = S.pack_split_on_device(params)
    assert split.numel() == S.split_train_floats()
    host = S.pack_split_host(T.pack_on_device(params).cpu().numpy())
    assert np.array_equal(split.cpu().numpy().view(np.uint32), host.view(np.uint32))
    assert S.pack_split_on_device(params) is split            # cached while no parameter is modified
    before = split.clone()
    for p in params:
        p.grad = torch.ones_like(p)
    torch.optim.SGD(params, lr=0.25).step()                   # in place: the versions move
    again = S.pack_split_on_device(params)
    assert again is not split and not torch.equal(again, before)
    host = S.pack_split_host(T.pack_on_device(params).cpu().numpy())
    assert np.array_equal(again.cpu().numpy().view(np.uint32), host.view(np.uint32))
