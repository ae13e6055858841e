"""Training path of the LIIF comparison decoder (liif.py:59-127 under autograd; diinn_amd.liif_training; opt-in LIIF.hip_autograd).

CPU part: the fixture set (tests/golden/liif_golden_grad_<case>.npz, from the REAL reference's autograd) and its input condition;
``liif_backward_reference`` (the formula sheet) in fp32 and float64 against the fixtures; ``masks=``; the gather index of the
device-side image; the refusals.
GPU part: ``modules.LIIF`` with ``hip_autograd`` under autograd on the HIP kernels against the fixtures; the mask-conditioned check
of the fused backward against the formula sheet in float64 at B = 2, 12x10 -> 31x27; ``diinn_liif_cell_sum`` alone; determinism and
``needs_input_grad``; ``SRLitModule(arch="liif")``; the switch off."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import diinn_amd.synth as synth

HERE = os.path.dirname(os.path.abspath(__file__))
ROW_STRIDE = 8
CASES = ["b2_3x2_5x4", "b1_4x3_9x7", "b1_8x8_5x6_down", "b1_1x1_7x5", "b1_2x3_8x12_gain2"]
PNAMES = [f"layers.{i}.{t}" for i in (0, 2, 4, 6, 8) for t in ("weight", "bias")]
IMNET_SHAPES = {"imnet.layers.0.weight": (256, 580), "imnet.layers.0.bias": (256,),
                **{f"imnet.layers.{i}.weight": (256, 256) for i in (2, 4, 6)}, **{f"imnet.layers.{i}.bias": (256,) for i in (2, 4, 6)},
                "imnet.layers.8.weight": (3, 256), "imnet.layers.8.bias": (3,)}
RTOL = 1e-4                      # the project's gradient bound: max|g - ref| <= 1e-4 max|ref| per tensor (tests/test_training_modes12.py)

_gold = {}


def gold(name):
    if name not in _gold:
        _gold[name] = np.load(os.path.join(HERE, "golden", f"liif_golden_grad_{name}.npz"))
    return _gold[name]


def _weights(seed, gain):
    sd = synth.state_dict_for(IMNET_SHAPES, seed, "liif.", gain=gain)
    return [sd["imnet." + n] for n in PNAMES]


def _inputs(name):
    b, h, w, hu, wu, gain, seed = gold(name)["meta"]
    b, h, w, hu, wu, seed = int(b), int(h), int(w), int(hu), int(wu), int(seed)
    feat = synth.encoder_features(seed, b, h, w)
    r = synth.uniform(seed, f"gradw:liif:{name}", (b, 3, hu, wu), 1.0)
    return _weights(seed, float(gain)), feat, r, (b, h, w, hu, wu)


def _check_against_fixture(name, d_feat, grads, rtol, tag=""):
    """max|g - ref| <= rtol * max|ref| per tensor (layers.0.weight: every 8th row is pinned).  ``rtol`` may be a function of the
    tensor's name."""
    g = gold(name)
    for pname, x in [("feat", d_feat)] + list(zip(PNAMES, grads)):
        ref = g[f"grad/{pname}"]
        x = np.asarray(x)
        if pname == "layers.0.weight":
            x = x[::ROW_STRIDE]
        assert x.shape == ref.shape, (pname, x.shape, ref.shape)
        err = float(np.abs(x.astype(np.float64) - ref).max())
        bound = rtol(pname) if callable(rtol) else rtol * max(float(np.abs(ref).max()), 1e-6)
        print(f"{name} {tag} {pname}: err {err:.3e} / max|ref| {float(np.abs(ref).max()):.3e} (bound {bound:.3e})")
        assert err <= bound, f"{name} {tag} {pname} err {err:.3e} > {bound:.3e}"


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------
def test_fixture_set_and_input_condition():
    """The five cases of the issue, each file below 1 MiB, dtypes as listed, and the stored min|a| over the four hidden layers'
    pre-activations meets the generator's condition min|a| >= 2e-6 * gain (no ReLU mask can flip under a few ulp of reordering)."""
    import glob
    files = sorted(glob.glob(os.path.join(HERE, "golden", "liif_golden_grad_*.npz")))
    names = [os.path.basename(f)[len("liif_golden_grad_"):-len(".npz")] for f in files]
    assert sorted(names) == sorted(CASES)
    for f, name in zip(files, names):
        assert os.path.getsize(f) < (1 << 20)
        g = gold(name)
        gain, seed = float(g["meta"][5]), int(g["meta"][6])
        assert seed >= 123
        assert float(g["min_abs_a"]) >= 2e-6 * gain, (name, float(g["min_abs_a"]))
        for key in ["out", "grad/feat"] + [f"grad/{p}" for p in PNAMES]:
            assert g[key].dtype == np.float32
        for key in ["out", "feat"] + PNAMES:
            assert g[f"d64/{key}"].shape == (2,) and g[f"d64/{key}"].dtype == np.float64
        assert g["grad/layers.0.weight"].shape == (256 // ROW_STRIDE, 580)


@pytest.mark.parametrize("name", CASES)
def test_formula_sheet_fp32_on_cpu(name):
    """liif_backward_reference (and the hoisted forward) in fp32 against the real reference's output and gradients."""
    import diinn_amd.liif_training as LT
    ws, feat, r, (b, h, w, hu, wu) = _inputs(name)
    params = [torch.from_numpy(x) for x in ws]
    out = LT.liif_forward_reference(torch.from_numpy(feat), params, (hu, wu)).numpy()
    ref_out = gold(name)["out"]
    assert float(np.abs(out - ref_out).max()) <= 1e-5 * max(1.0, float(np.abs(ref_out).max()))
    d_feat, grads = LT.liif_backward_reference(torch.from_numpy(r), torch.from_numpy(feat), params, (hu, wu))
    assert d_feat.dtype == torch.float32
    _check_against_fixture(name, d_feat.numpy(), [g.numpy() for g in grads], RTOL, "formula fp32")


@pytest.mark.parametrize("name", CASES)
def test_formula_sheet_float64_on_cpu(name):
    """liif_backward_reference in float64 is within 1e-6 * max of the reference's float64 gradients.  The fixtures hold the
    reference's fp32 gradients and d64 = [max|fp32 - float64|, max|float64|], so by the triangle inequality
    |formula64 - ref32| <= d64[0] + 1e-6 * d64[1] per tensor."""
    import diinn_amd.liif_training as LT
    ws, feat, r, (b, h, w, hu, wu) = _inputs(name)
    params = [torch.from_numpy(x).double() for x in ws]
    d_feat, grads = LT.liif_backward_reference(torch.from_numpy(r).double(), torch.from_numpy(feat).double(), params, (hu, wu))
    assert d_feat.dtype == torch.float64 and all(g.dtype == torch.float64 for g in grads)
    d64 = gold(name)
    _check_against_fixture(name, d_feat.numpy(), [g.numpy() for g in grads],
                           lambda p: float(d64[f"d64/{p}"][0]) + 1e-6 * float(d64[f"d64/{p}"][1]), "formula f64")
    no_feat, _ = LT.liif_backward_reference(torch.from_numpy(r), torch.from_numpy(feat), [torch.from_numpy(x) for x in ws], (hu, wu),
                                            need_feat_grad=False)
    assert no_feat is None


def test_masks_argument_reproduces_the_formula_sheets_own_masks():
    """Passing [a_l > 0] of the formula sheet's own pre-activations as ``masks=`` reproduces ``masks=None`` exactly; other masks
    change the result."""
    import diinn_amd.liif_training as LT
    ws, feat, r, (b, h, w, hu, wu) = _inputs("b1_4x3_9x7")
    params = [torch.from_numpy(x) for x in ws]
    ft, rt = torch.from_numpy(feat), torch.from_numpy(r)
    pre = LT.liif_preactivations(ft, params, (hu, wu))
    assert len(pre) == 4 and all(tuple(a.shape) == (4, b * hu * wu, 256) for a in pre)
    d0, g0 = LT.liif_backward_reference(rt, ft, params, (hu, wu))
    d1, g1 = LT.liif_backward_reference(rt, ft, params, (hu, wu), masks=[a > 0 for a in pre])
    assert torch.equal(d0, d1) and all(torch.equal(x, y) for x, y in zip(g0, g1))
    d2, _ = LT.liif_backward_reference(rt, ft, params, (hu, wu), masks=[torch.ones_like(a, dtype=torch.bool) for a in pre])
    assert not torch.equal(d0, d2)


def test_gather_index_reproduces_the_host_packer():
    """The device-side gather index reproduces pack_liif_state_dict exactly on a synthetic state dict in every section a LIIF kernel
    reads (all but the derived, inference-only sections of the DIINN image and its validity word, which the index leaves zero),
    and references every parameter element."""
    import diinn_amd._native as N
    import diinn_amd.decoder as D
    import diinn_amd.liif_training as LT
    ws = _weights(5, 1.0)
    host = D.pack_liif_state_dict({n: x for n, x in zip(PNAMES, ws)}, prefix="").numpy()
    idx = LT.pack_gather_index().numpy()
    assert idx.shape == host.shape
    flat = np.concatenate([x.reshape(-1) for x in ws] + [np.zeros(1, np.float32)])
    got = flat[idx]
    lib = N.load()
    derived = np.zeros(host.size, bool)
    off, size = C.c_size_t(), C.c_size_t()
    for section in LT.DERIVED_SECTIONS:
        assert lib.diinn_packed_section(section, C.byref(off), C.byref(size)) == 0
        derived[off.value:off.value + size.value] = True
    assert lib.diinn_packed_section(6, C.byref(off), C.byref(size)) == 0
    derived[off.value + 3] = True
    assert np.array_equal(got[~derived], host[~derived])
    assert not got[derived].any()
    assert np.unique(idx[idx < flat.size - 1]).size == flat.size - 1
    # the image on a device is that gather (CPU tensors stand in for the device here)
    image = LT.image_on_device([torch.from_numpy(x) for x in ws])
    assert np.array_equal(image.numpy(), got)


def test_refusals_on_cpu():
    """Switch off: LIIF under grad raises NotImplementedError and the message names the switch.  Switch on with a CPU tensor: the
    usual "ROCm GPU" RuntimeError, no fallback (attribute and constructor keyword alike)."""
    import diinn_amd.liif_training as LT
    import diinn_amd.modules as M
    x = torch.rand(1, 3, 6, 5)
    net = M.LIIF().train()
    assert net.hip_autograd is False
    with pytest.raises(NotImplementedError, match="hip_autograd"):
        net(x, (13, 11))
    net.hip_autograd = True
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        net(x, (13, 11))
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        M.LIIF(hip_autograd=True).train()(x, (13, 11))
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        LT.decode_with_grad(net.imnet, torch.rand(1, 64, 6, 5, requires_grad=True), (13, 11))


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
class _GivenFeatures(torch.nn.Module):
    """Stands in for the encoder: returns the given feature map (a leaf that requires grad)."""

    out_dim = 64

    def __init__(self, feat):
        super().__init__()
        self.feat = feat

    def forward(self, inp):
        return self.feat


def _model(ws, dev, **kw):
    import diinn_amd.modules as M
    net = M.LIIF(**kw)
    net.imnet.load_state_dict({n: torch.from_numpy(x) for n, x in zip(PNAMES, ws)}, strict=True)
    return net.to(dev).train()


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_liif_autograd_against_reference_fixtures(name):
    """modules.LIIF.forward with hip_autograd under autograd (bsize=None) on given features: the output is the no_grad output bit
    for bit and within 1e-5 of the reference's; with bsize the output carries no graph and is equal; every gradient is within
    1e-4 * max|ref| of the reference's own .grad."""
    dev = torch.device("cuda:0")
    ws, feat, r, (b, h, w, hu, wu) = _inputs(name)
    net = _model(ws, dev)
    net.hip_autograd = True
    x = torch.from_numpy(feat).to(dev).requires_grad_(True)
    net.encoder = _GivenFeatures(x)
    inp = torch.zeros((b, 3, h, w), device=dev)
    y = net(inp, (hu, wu))
    assert y.requires_grad
    with torch.no_grad():
        y0 = net(inp, (hu, wu))
    assert torch.equal(y.detach(), y0)
    yb = net(inp, (hu, wu), 300)                                  # bsize: the reference's no_grad decode
    assert not yb.requires_grad and torch.equal(yb, y0)
    ref_out = gold(name)["out"]
    assert float(np.abs(y0.cpu().numpy() - ref_out).max()) <= 1e-5 * max(1.0, float(np.abs(ref_out).max()))
    (y * torch.from_numpy(r).to(dev)).sum().backward()
    named = dict(net.imnet.named_parameters())
    _check_against_fixture(name, x.grad.cpu().numpy(), [named[n].grad.cpu().numpy() for n in PNAMES], RTOL, "hip")


@pytest.mark.gpu
def test_fused_backward_given_the_forwards_masks():
    """B = 2, 12x10 -> 31x27, seed 123: 1,674 pixels, 6,696 virtual pixels = 209.25 plane tiles, 240 cells = 7.5 tiles.  At this
    size some pre-activation lies within fp32 noise of zero whatever the seed, so the masks are taken from the HIP forward's saved
    planes and
    (a) they equal the float64 formula sheet's masks except where |a64| <= 4 * max|a32 - a64| of that layer (a32: the fp32 formula
        sheet's pre-activation on the same device, not the code under test; the factor 4 covers a differently ordered 256-term
        sum); the set so excused is below 1e-4 of all values;
    (b) the fused gradients are within 1e-4 * max|g64| per tensor of liif_backward_reference in float64 GIVEN those masks.
    Recorded, not asserted: the fp32 formula sheet's own distance."""
    import diinn_amd.liif_training as LT
    dev = torch.device("cuda:0")
    b, h, w, hu, wu, seed = 2, 12, 10, 31, 27, 123
    n = b * hu * wu
    assert (4 * n) % 32 == 8 and (b * h * w) % 32 == 16
    ws = _weights(seed, 1.0)
    feat = torch.from_numpy(synth.encoder_features(seed, b, h, w)).to(dev)
    r = torch.from_numpy(synth.uniform(seed, "gradw:liif:masks", (b, 3, hu, wu), 1.0)).to(dev)
    params = [torch.from_numpy(x).to(dev).requires_grad_(True) for x in ws]
    x = feat.clone().requires_grad_(True)
    image = LT.image_on_device(params)
    out_f, acts = LT.train_forward(feat.contiguous(), image, hu, wu)
    saved = LT.saved_activations(acts, b, hu, wu)                 # [4 members][4 layers][256][N]
    assert tuple(saved.shape) == (4, 4, 256, n)
    masks = [(saved[:, l] > 0).permute(0, 2, 1).contiguous() for l in range(4)]          # per layer [4, N, 256]
    p64 = [p.detach().double() for p in params]
    a64 = LT.liif_preactivations(feat.double(), p64, (hu, wu))
    a32 = LT.liif_preactivations(feat, [p.detach() for p in params], (hu, wu))
    excused_total = 0
    for l in range(4):
        tol = 4.0 * float((a32[l].double() - a64[l]).abs().max())
        excused = a64[l].abs() <= tol
        differ = masks[l] != (a64[l] > 0)
        print(f"layer {l + 1}: {int(differ.sum())} masks differ from float64, {int(excused.sum())} of {excused.numel()} excused (|a64| <= {tol:.3e})")
        assert not bool((differ & ~excused).any())
        excused_total += int(excused.sum())
        # the saved planes are the activations themselves
        err_h = float((saved[:, l].permute(0, 2, 1).double() - torch.relu(a64[l])).abs().max())
        assert err_h <= 1e-5 * max(1.0, float(a64[l].abs().max())), (l, err_h)
    assert excused_total < 1e-4 * 4 * a64[0].numel()
    y = LT.LIIFFunction.apply(x, hu, wu, *params)
    assert torch.equal(y.detach(), out_f)
    (y * r).sum().backward()
    d64_feat, g64 = LT.liif_backward_reference(r.double(), feat.double(), p64, (hu, wu), masks=masks)
    d32_feat, g32 = LT.liif_backward_reference(r, feat, [p.detach() for p in params], (hu, wu), masks=masks)
    for pname, got, f32, ref in zip(["feat"] + PNAMES, [x.grad] + [p.grad for p in params], [d32_feat] + g32, [d64_feat] + g64):
        err = float((got.double() - ref).abs().max())
        own = float((f32.double() - ref).abs().max())
        scale = float(ref.abs().max())
        print(f"{pname}: fused err {err:.3e}, fp32 formula sheet {own:.3e}, max|f64| {scale:.3e} (bound {RTOL * scale:.3e})")
        assert err <= RTOL * scale, (pname, err, scale)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 12, 10, 31, 27), (1, 8, 8, 5, 6), (1, 16, 16, 3, 4)])
def test_cell_sum_kernel_alone(shape):
    """diinn_liif_cell_sum on random g_a,1 planes against an index_add_ in float64: 1e-5 * max|ref| (a cell sum has few terms); the
    tiled layout equals tile_planes of the NCHW one; unowned cells are exact zeros; rows >= 256 and the padding of the ragged last
    tiles are untouched (pre-filled with NaN; the padding of g_a,1 is NaN as well: never read); bad arguments return status 1.
    16x16 -> 3x4 is the shape where most cells own nothing."""
    import diinn_amd._native as N
    import diinn_amd.liif_training as LT
    import diinn_amd.training as T
    dev = torch.device("cuda:0")
    b, h, w, hu, wu = shape
    n, cells = b * hu * wu, b * h * w
    gen = torch.Generator(device=dev).manual_seed(11)
    g1 = torch.randn((256, 4 * n), device=dev, generator=gen)
    g1_t = T.tile_planes(g1)
    assert (4 * n) % 32 != 0
    g1_t[-1, :, (4 * n) % 32:] = float("nan")
    dp = torch.full((b, 1024, h, w), float("nan"), device=dev)
    dp_t = torch.full(((cells + 31) // 32, 1024, 32), float("nan"), device=dev)
    LT.cell_sum(g1_t, b, h, w, hu, wu, dp=dp, dp_t=dp_t)
    dp2, dp_t2 = LT.cell_sum(g1_t, b, h, w, hu, wu)
    torch.cuda.synchronize()
    assert torch.equal(dp[:, :256], dp2[:, :256])                 # deterministic
    cell, _, _ = LT._virtual_tables(b, h, w, hu, wu, dev, torch.float64)
    ref = torch.zeros((cells, 256), dtype=torch.float64, device=dev).index_add_(0, cell.reshape(-1), g1.t().double())
    got = dp[:, :256].permute(0, 2, 3, 1).reshape(cells, 256)
    assert float((got.double() - ref).abs().max()) <= 1e-5 * float(ref.abs().max())
    assert bool(torch.isnan(dp[:, 256:]).all()) and bool(torch.isnan(dp_t[:, 256:]).all())
    flat = dp[:, :256].permute(1, 0, 2, 3).reshape(256, cells)
    assert torch.equal(T.untile_planes(dp_t, cells)[:256], flat)
    if cells % 32:
        assert bool(torch.isnan(dp_t[-1, :, cells % 32:]).all())
        assert torch.equal(dp_t2[:, :256], T.tile_planes(flat))   # (the buffer the wrapper allocates: zero padding)
    owned = torch.zeros(cells, dtype=torch.bool, device=dev)
    owned[cell.reshape(-1)] = True
    print(f"{shape}: {int((~owned).sum())} of {cells} cells own no virtual pixel")
    if shape[1:] == (16, 16, 3, 4):                               # (at 8x8 -> 5x6 the four shifted members together reach every cell)
        assert int((~owned).sum()) > cells // 2
    assert not bool(got[~owned].any())
    lib = N.load()
    geo = LT._geometry(b, h, w, hu, wu, dev)
    ptr = lambda t: C.c_void_p(t.data_ptr())                      # noqa: E731
    assert lib.diinn_liif_cell_sum(None, None, ptr(geo["seg_h"]), ptr(geo["seg_w"]), ptr(dp), ptr(dp_t), b, h, w, hu, wu) == 1
    assert lib.diinn_liif_cell_sum(None, ptr(g1_t), ptr(geo["seg_h"]), ptr(geo["seg_w"]), ptr(dp), None, b, h, w, hu, wu) == 1
    assert lib.diinn_liif_cell_sum(None, ptr(g1_t), ptr(geo["seg_h"]), ptr(geo["seg_w"]), ptr(dp), ptr(dp_t), b, h, w, 0, wu) == 1
    assert lib.diinn_liif_backward_data(None, None, ptr(g1_t), ptr(g1_t), ptr(g1_t), b, h, w, hu, wu) == 1
    assert lib.diinn_liif_train_fwd(None, ptr(g1_t), ptr(g1_t), ptr(g1_t), ptr(dp), None, b, h, w, hu, wu) == 1


@pytest.mark.gpu
def test_backward_is_deterministic_and_honours_needs_input_grad():
    """Two backward passes are bit-identical; only ``feat.requires_grad`` and only some parameters requiring grad each return
    exactly that subset, with the values of the full pass (a frozen encoder skips d_feat, frozen layers.0 the conv's weight GEMM)."""
    import diinn_amd.liif_training as LT
    dev = torch.device("cuda:0")
    ws, feat, r, (b, h, w, hu, wu) = _inputs("b1_4x3_9x7")
    rr = torch.from_numpy(r).to(dev)

    def run(feat_grad, which):
        params = [torch.from_numpy(x).to(dev).requires_grad_(n in which) for n, x in zip(PNAMES, ws)]
        x = torch.from_numpy(feat).to(dev).requires_grad_(feat_grad)
        y = LT.LIIFFunction.apply(x, hu, wu, *params)
        (y * rr).sum().backward()
        return y.detach(), x.grad, [p.grad for p in params]

    y1, f1, g1 = run(True, PNAMES)
    y2, f2, g2 = run(True, PNAMES)
    assert torch.equal(y1, y2) and torch.equal(f1, f2) and all(torch.equal(a, c) for a, c in zip(g1, g2))
    _, f3, g3 = run(True, [])
    assert torch.equal(f3, f1) and all(g is None for g in g3)
    _, f4, g4 = run(False, ["layers.0.bias", "layers.4.weight", "layers.8.weight"])
    assert f4 is None
    for i, n in enumerate(PNAMES):
        if n in ("layers.0.bias", "layers.4.weight", "layers.8.weight"):
            assert torch.equal(g4[i], g1[i]), n
        else:
            assert g4[i] is None, n
    _, f5, g5 = run(False, ["layers.0.weight"])
    assert f5 is None and torch.equal(g5[0], g1[0]) and all(g is None for g in g5[1:])


@pytest.mark.gpu
def test_srlitmodule_liif_training_steps():
    """Five Adam steps of SRLitModule(arch="liif").step with the switch on (``net.net.hip_autograd = True``) on a 12x10 image at two
    scales: finite, decreasing loss; afterwards an eval forward follows the updated weights (the host-packed inference image is
    rebuilt): it equals the formula sheet on the updated weights within the forward tolerance and, bit for bit, the decoder
    output under grad on the same features (the image gathered on the device is rebuilt too)."""
    import diinn_amd.liif_training as LT
    import diinn_amd.modules as M
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    net = M.SRLitModule(arch="liif").to(dev).train()
    net.net.hip_autograd = True
    opt = torch.optim.Adam(net.parameters(), lr=1e-4)
    lr = torch.rand(2, 3, 12, 10, device=dev)
    batch = {2: (lr, torch.rand(2, 3, 24, 20, device=dev), ["a", "b"]),
             3: (lr, torch.rand(2, 3, 31, 27, device=dev), ["a", "b"])}
    before = [p.detach().clone() for p in net.net.imnet.parameters()]
    losses = []
    for _ in range(5):
        opt.zero_grad(set_to_none=True)
        loss, _ = net.step(batch)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert all(np.isfinite(losses))
    assert losses[-1] < losses[0], losses
    assert all(not torch.equal(p.detach(), q) for p, q in zip(net.net.imnet.parameters(), before))
    x = (lr - net.sub) / net.div
    net.eval()
    named = dict(net.net.imnet.named_parameters())
    with torch.no_grad():
        y_eval = net.net(x, (31, 27))
        feat = net.net.gen_feat(x)
        want = LT.liif_forward_reference(feat.double(), [named[n].double() for n in PNAMES], (31, 27))
    assert float((y_eval.double() - want).abs().max()) <= 1e-5 * max(1.0, float(want.abs().max()))
    xg = feat.clone().requires_grad_(True)
    y = LT.decode_with_grad(net.net.imnet, xg, (31, 27))
    assert torch.equal(y.detach(), y_eval)                        # (the image gathered on the device == the host-packed one)
    y.sum().backward()
    assert bool(torch.isfinite(xg.grad).all()) and float(xg.grad.abs().max()) > 0


@pytest.mark.gpu
def test_switch_off_still_raises_on_the_gpu():
    """With LIIF.hip_autograd unset (the default) a call under grad raises NotImplementedError, as before the training path."""
    dev = torch.device("cuda:0")
    ws = _weights(123, 1.0)
    net = _model(ws, dev)
    assert net.hip_autograd is False
    with pytest.raises(NotImplementedError, match="hip_autograd"):
        net(torch.rand(1, 3, 12, 10, device=dev), [31, 27])
    with torch.no_grad():
        assert tuple(net(torch.rand(1, 3, 12, 10, device=dev), [31, 27]).shape) == (1, 3, 31, 27)
