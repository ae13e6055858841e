"""Training path of decoder modes 1 and 2 (diinn.py:116-131 under autograd): the modulation chain lives on the LR cells.

CPU part: ``training.backward_from_saved_modes12`` (the formula sheet) fed with planes computed from the oracle's pieces,
against the REAL reference's .grad fixtures (tests/golden/diinn_golden_grad_m12_<case>.npz); the mode-aware gather index.
GPU part: ``ImplicitDecoder(mode=1|2)`` under autograd on the HIP kernels against the fixtures and a float64 autograd run
of the oracle's step; the fused backward against the formula sheet; ``diinn_cell_chain_bwd`` alone; the bias pitfall; mode 1's
shapes; ``SRLitModule.step``; determinism."""
import ctypes as C
import glob
import os

import numpy as np
import pytest
import torch

import diinn_amd.synth as synth
import diinn_oracle as orc

HERE = os.path.dirname(os.path.abspath(__file__))
ROW_STRIDE = 8
MODES = (1, 2)
CASE_FILES = sorted(glob.glob(os.path.join(HERE, "golden", "diinn_golden_grad_m12_*.npz")))
CASE_NAMES = [os.path.basename(f)[len("diinn_golden_grad_m12_"):-len(".npz")] for f in CASE_FILES]
STRESS = "b1_9x14_36x56_stress"


def test_fixture_cases_are_the_four_of_the_issue():
    assert sorted(CASE_NAMES) == sorted(["b2_12x10_31x27", STRESS, "b1_8x8_5x6_down", "b1_1x1_7x5"])
    for f in CASE_FILES:
        assert os.path.getsize(f) < (1 << 20)


_gold = {}


def gold(name):
    if name not in _gold:
        _gold[name] = np.load(os.path.join(HERE, "golden", f"diinn_golden_grad_m12_{name}.npz"))
    return _gold[name]


def _inputs(name, m):
    b, h, w, hu, wu, gain = gold(name)["meta"]
    b, h, w, hu, wu = int(b), int(h), int(w), int(hu), int(wu)
    sd = synth.decoder_state_dict(123, float(gain), mode=m)
    feat = synth.encoder_features(123, b, h, w)
    r = synth.uniform(123, f"gradw:m{m}:{name}", (b, 3, hu, wu), 1.0)
    return sd, feat, r, (b, h, w, hu, wu)


def _strided(pname):
    return pname[0] in "KQ" and pname.endswith("weight")


def _check_against_fixture(name, m, d_feat, grads, rtol):
    """max|g - ref| <= rtol * max|ref| per tensor (K and Q weights: every 8th output row is pinned)."""
    g = gold(name)
    ref = g[f"grad/m{m}/feat"]
    err = float(np.abs(d_feat - ref).max())
    print(f"{name} m{m} d_feat: err {err:.3e} / max|ref| {float(np.abs(ref).max()):.3e}")
    assert err <= rtol * max(float(np.abs(ref).max()), 1e-6), f"{name} m{m} d_feat err {err:.3e}"
    for pname, x in grads.items():
        ref = g[f"grad/m{m}/{pname}"]
        if _strided(pname):
            x = x[::ROW_STRIDE]
        assert x.shape == ref.shape, (pname, x.shape, ref.shape)
        err = float(np.abs(x - ref).max())
        print(f"{name} m{m} {pname}: err {err:.3e} / max|ref| {float(np.abs(ref).max()):.3e}")
        assert err <= rtol * max(float(np.abs(ref).max()), 1e-6), f"{name} m{m} {pname} err {err:.3e}"


_truth = {}


def truth64(name, m):
    """(out, d_feat, {name: grad}) of a float64 autograd run of the oracle's step for decoder mode m; computed once."""
    if (name, m) not in _truth:
        sd, feat, r, (b, h, w, hu, wu) = _inputs(name, m)
        params = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in sd.items()}
        f = torch.from_numpy(feat).double().requires_grad_(True)
        syn, idx_h, idx_w = orc.make_syn_inp(b, h, w, hu, wu)
        u = orc.unfold3x3(f)
        x = u[:, :, torch.from_numpy(idx_h.astype(np.int64))][:, :, :, torch.from_numpy(idx_w.astype(np.int64))]
        out = orc._step_mode3(params, x, syn.double(), m)
        (out * torch.from_numpy(r).double()).sum().backward()
        _truth[(name, m)] = (out.detach(), f.grad, {k: v.grad for k, v in params.items()})
    return _truth[(name, m)]


@torch.no_grad()
def saved_planes_m12(sd, feat, size, m):
    """What cell_chain_kernel and decode_kernel<KPART=false, SAVE> leave, restated on the CPU in fp32 from the oracle's pieces:
    the chain k_i on the LR cells ([4, 256, B*H*W]; as the kernels do, and unlike the reference, which runs it on the replicated
    map: same numbers, computed once per cell), and the planes acts[i, 0] = k_i of the pixel's cell, acts[i, 1] = s_i as
    [256, B*Hu*Wu]; plus the decoder output."""
    sd = {k: torch.from_numpy(v) for k, v in sd.items()}
    f = torch.from_numpy(feat)
    b, c, h, w = f.shape
    hu, wu = size
    syn, idx_h, idx_w = orc.make_syn_inp(b, h, w, hu, wu)
    ih, iw = torch.from_numpy(idx_h.astype(np.int64)), torch.from_numpy(idx_w.astype(np.int64))
    u = orc.unfold3x3(f)                                          # [B,576,H,W]
    n, cells = b * hu * wu, b * h * w
    acts = torch.empty((4, 2, 256, n))
    cell_k = torch.empty((4, 256, cells))
    plane = lambda t: t.permute(1, 0, 2, 3).reshape(256, -1)      # noqa: E731
    up = lambda t: t[:, :, ih][:, :, :, iw]                       # noqa: E731  nearest-exact replication (diinn.py:168)
    k = torch.relu(orc._conv1x1(u, sd["K.0.0.weight"], sd["K.0.0.bias"]))
    s = orc._conv1x1(syn, sd["Q.0.0.weight"], sd["Q.0.0.bias"])
    cell_k[0], acts[0, 0], acts[0, 1] = plane(k), plane(up(k)), plane(s)
    q = up(k) * torch.sin(s)
    for i in range(1, 4):
        k = torch.relu(orc._conv1x1(torch.cat([k, u], dim=1) if m == 2 else k, sd[f"K.{i}.0.weight"], sd[f"K.{i}.0.bias"]))
        s = orc._conv1x1(q, sd[f"Q.{i}.0.weight"], sd[f"Q.{i}.0.bias"])
        cell_k[i], acts[i, 0], acts[i, 1] = plane(k), plane(up(k)), plane(s)
        q = up(k) * torch.sin(s)
    return orc._conv1x1(q, sd["last_layer.weight"], sd["last_layer.bias"]), acts, cell_k


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("m", MODES)
@pytest.mark.parametrize("name", CASE_NAMES)
def test_backward_formulas_modes12_on_cpu(name, m):
    """training.backward_from_saved_modes12 with oracle-computed saved planes against the real reference's gradients, at the
    bound of the mode-3 formula test (5e-5 of max|ref| per tensor)."""
    import diinn_amd.training as T
    sd, feat, r, (b, h, w, hu, wu) = _inputs(name, m)
    out, acts, cell_k = saved_planes_m12(sd, feat, (hu, wu), m)
    ref_out = gold(name)[f"out/m{m}"]
    assert float(np.abs(out.numpy() - ref_out).max()) <= 1e-5 * max(1.0, float(np.abs(ref_out).max()))
    shapes = T.param_shapes(m)
    params = [torch.from_numpy(sd[n]) for n in T.PARAM_NAMES]
    d_feat, d_params = T.backward_from_saved_modes12(torch.from_numpy(r), torch.from_numpy(feat), acts, params, (hu, wu), m,
                                                     cell_k=cell_k)
    # the chain recomputed by the formula sheet itself (plain conv + matmul) is the same chain
    ck = T.cell_chain_planes(torch.from_numpy(feat), params, m)
    assert float((ck - cell_k).abs().max()) <= 1e-5 * max(1.0, float(cell_k.abs().max()))
    grads = {n: g.numpy() for n, g in zip(T.PARAM_NAMES, d_params)}
    for n in T.PARAM_NAMES:
        assert grads[n].shape == tuple(shapes[n]) == sd[n].shape, n
    _check_against_fixture(name, m, d_feat.numpy(), grads, 5e-5)


@pytest.mark.parametrize("m", MODES)
def test_gather_index_modes12_is_the_host_packer(m):
    """The mode-aware device re-pack: a permutation of the parameter elements plus references to the appended zero; every
    parameter element is referenced; outside the derived sections the gather reproduces diinn_pack_weights(mode)."""
    import diinn_amd._native as N
    import diinn_amd.decoder as D
    import diinn_amd.training as T
    lib = N.load()
    sd = synth.decoder_state_dict(7, mode=m)
    shapes = T.param_shapes(m)
    assert shapes["K.1.0.weight"] == ((256, 256, 1, 1) if m == 1 else (256, 832, 1, 1))
    total = sum(int(np.prod(shapes[n])) for n in T.PARAM_NAMES)
    idx = T.pack_gather_index(m).numpy()
    assert idx.shape == (lib.diinn_packed_weight_floats(),) and idx.min() >= 0 and idx.max() == total
    assert np.array_equal(np.unique(idx[idx < total]), np.arange(total))          # every element referenced
    if m == 2:
        assert np.array_equal(idx, T.pack_gather_index(3).numpy())                # modes 2 and 3 share the layout
    flat = torch.cat([torch.from_numpy(sd[n]).reshape(-1) for n in T.PARAM_NAMES] + [torch.zeros(1)])
    got = flat[torch.from_numpy(idx)].numpy()
    ref = D.pack_state_dict(sd, mode=m).numpy()
    off, size = C.c_size_t(), C.c_size_t()
    keep = np.ones(ref.size, bool)
    for section in (7, 9, 10, 11, 12, 13, 14, 15, 16):
        assert lib.diinn_packed_section(section, C.byref(off), C.byref(size)) == 0
        keep[off.value:off.value + size.value] = False
    assert lib.diinn_packed_section(6, C.byref(off), C.byref(size)) == 0
    keep[off.value + 3] = False                                                   # the validity word
    assert np.array_equal(got[keep], ref[keep]) and not got[~keep].any()
    if m == 1:
        # the zero feature columns of the widened K.1..3 point at the appended zero: layers 1..3 of the hoisted conv (section 1)
        assert lib.diinn_packed_section(1, C.byref(off), C.byref(size)) == 0
        wp = idx[off.value:off.value + size.value]
        assert int((wp == total).sum()) == 3 * 256 * 576 and int((wp < total).sum()) == 256 * 576


def test_refusals_stay_notimplemented_before_the_device():
    import diinn_amd.decoder as D
    for kw in (dict(mode=4), dict(mode=1, compute="bf16"), dict(mode=2, compute="bf16x3"), dict(mode=3, compute="bf16")):
        with pytest.raises(NotImplementedError, match="autograd"):
            D.ImplicitDecoder(init_q=False, **kw)(torch.zeros(1, 64, 4, 4), (8, 8))
    with pytest.raises(RuntimeError, match="ROCm GPU"):                            # modes 1/2 are routed on: the CPU tensor is refused
        D.ImplicitDecoder(mode=1, init_q=False)(torch.zeros(1, 64, 4, 4), (8, 8))


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
_runs = {}


def gpu_run(name, m):
    """One forward + backward of ImplicitDecoder(mode=m) on the HIP path; (out, d_feat, {name: grad}) as numpy, computed once."""
    if (name, m) not in _runs:
        import diinn_amd.decoder as D
        dev = torch.device("cuda:0")
        sd, feat, r, (b, h, w, hu, wu) = _inputs(name, m)
        dec = D.ImplicitDecoder(mode=m, init_q=False)
        dec.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
        dec = dec.to(dev).train()
        x = torch.from_numpy(feat).to(dev).requires_grad_(True)
        y = dec(x, [hu, wu])
        (y * torch.from_numpy(r).to(dev)).sum().backward()
        torch.cuda.synchronize()
        _runs[(name, m)] = (y.detach().cpu().numpy(), x.grad.cpu().numpy(), {n: p.grad.cpu().numpy() for n, p in dec.named_parameters()})
    return _runs[(name, m)]


@pytest.mark.gpu
@pytest.mark.parametrize("m", MODES)
@pytest.mark.parametrize("name", CASE_NAMES)
def test_autograd_through_hip_decoder_modes12(name, m):
    """dec = ImplicitDecoder(mode=m).train(); y = dec(x.requires_grad_(), size); (y * R).sum().backward(): y at the decoder
    contract, every gradient against the real reference's fp32 fixture and (full tensors) the float64 oracle, both at the
    project's gradient bound max|g - ref| <= 1e-4 max|ref| per tensor.  On the parent commit forward raises NotImplementedError."""
    y, d_feat, grads = gpu_run(name, m)
    ref_out = gold(name)[f"out/m{m}"]
    err = np.abs(y - ref_out)
    print(f"{name} m{m} out: err {float(err.max()):.3e}")
    assert bool((err <= 1e-4 * np.maximum(1.0, np.abs(ref_out))).all())
    _check_against_fixture(name, m, d_feat, grads, 1e-4)
    _, f64, g64 = truth64(name, m)
    g = gold(name)
    for n, x in grads.items():
        ref = g64[n].numpy()
        assert x.shape == ref.shape, n
        err = float(np.abs(x - ref).max())
        d = g[f"d64/m{m}/{n}"]
        print(f"{name} m{m} {n}: |gpu - f64| / max|f64| = {err / max(float(np.abs(ref).max()), 1e-30):.2e}   (reference fp32: {d[0] / max(d[1], 1e-30):.2e})")
        assert err <= 1e-4 * max(float(np.abs(ref).max()), 1e-6), n
    err = float(np.abs(d_feat - f64.numpy()).max())
    d = g[f"d64/m{m}/feat"]
    print(f"{name} m{m} d_feat: |gpu - f64| / max|f64| = {err / float(f64.abs().max()):.2e}   (reference fp32: {d[0] / d[1]:.2e})")
    assert err <= 1e-4 * float(f64.abs().max())


@pytest.mark.gpu
@pytest.mark.parametrize("m", MODES)
def test_chain_bias_gradients_are_sums_over_cells(m):
    """The bias pitfall: dbK_i is the sum over CELLS of the chained gradient g_a,i, not the pixel row-sum of g^_a,i the plane
    GEMM's row-sum column gives in mode 3.  Gain 3 (mixed masks), against float64."""
    _, _, grads = gpu_run(STRESS, m)
    _, _, g64 = truth64(STRESS, m)
    for i in (1, 2, 3):
        ref = g64[f"K.{i}.0.bias"].numpy()
        err = float(np.abs(grads[f"K.{i}.0.bias"] - ref).max())
        print(f"m{m} K.{i}.0.bias: err {err:.3e} / max|ref| {float(np.abs(ref).max()):.3e}")
        assert float(np.abs(ref).max()) > 0
        assert err <= 1e-4 * float(np.abs(ref).max())


@pytest.mark.gpu
def test_mode1_shapes_and_feature_gradient():
    """Mode 1: K.i.weight.grad is [256,256,1,1]; only layer 0 reaches the features, and d_feat equals the float64 truth."""
    for name in ("b2_12x10_31x27", STRESS):
        _, d_feat, grads = gpu_run(name, 1)
        _, f64, g64 = truth64(name, 1)
        for i in (1, 2, 3):
            assert grads[f"K.{i}.0.weight"].shape == (256, 256, 1, 1)
        assert grads["K.0.0.weight"].shape == (256, 576, 1, 1)
        assert float(np.abs(d_feat - f64.numpy()).max()) <= 1e-4 * float(f64.abs().max())
    # only layer 0 reaches the features: the hoisted conv of mode 1 is K.0's 256 rows alone
    import diinn_amd.training as T
    sd, _, _, _ = _inputs("b1_8x8_5x6_down", 1)
    assert T._hoisted_conv_weight({n: torch.from_numpy(sd[n]) for n in T.PARAM_NAMES}, 1).shape == (256, 64, 3, 3)


@pytest.mark.gpu
@pytest.mark.parametrize("m", MODES)
def test_fused_backward_equals_formula_backward_modes12(m):
    """backward_fused_modes12 (bwd_layer_kernel<., KPART=false>, cell sums, cell_chain_bwd_kernel, plane GEMMs / rowdots, the conv
    gradients on the library's kernels) against backward_from_saved_modes12 on the SAME saved planes and chain workspace: a shape
    with ragged pixel and cell tiles, and a down-scaling one whose cells mostly own no pixel."""
    import diinn_amd.training as T
    dev = torch.device("cuda:0")
    for (b, h, w, hu, wu, gain) in [(3, 17, 13, 50, 41, 1.0), (2, 5, 40, 3, 9, 3.0)]:
        sd = synth.decoder_state_dict(5, gain, mode=m)
        feat = torch.from_numpy(synth.encoder_features(5, b, h, w)).to(dev)
        params = [torch.from_numpy(sd[n]).to(dev) for n in T.PARAM_NAMES]
        gout = torch.from_numpy(synth.uniform(5, "g", (b, 3, hu, wu), 1.0)).to(dev)
        n, cells = b * hu * wu, b * h * w
        out, acts_t, chain, packed = T.train_forward_modes12(feat, params, hu, wu, 2, m)
        torch.cuda.synchronize()
        acts = T.untile_planes(acts_t, n).view(4, 2, 256, n)
        assert torch.isfinite(acts).all()
        ck = chain.view(cells, 4, 256).permute(1, 2, 0)                       # [4, 256, cells]
        cell_k = torch.relu(ck)
        # the saved k planes are the chain's k_i of the pixel's cell, replicated
        idx_h, _, idx_w, _, _ = T.coordinate_tensors(h, w, hu, wu, dev)
        cell_of = ((torch.arange(b, device=dev)[:, None, None] * h + idx_h[None, :, None]) * w + idx_w[None, None, :]).reshape(-1)
        assert torch.equal(acts[:, 0], cell_k[:, :, cell_of])
        # the formula sheet's own chain (plain conv + matmul) agrees with the kernels' workspace
        ck_ref = T.cell_chain_planes(feat, params, m)
        assert float((cell_k - ck_ref).abs().max()) <= 2e-5 * max(1.0, float(ck_ref.abs().max()))
        df_a, dp_a = T.backward_fused_modes12(gout, feat, acts_t, chain, params, packed, (hu, wu), m)
        df_b, dp_b = T.backward_from_saved_modes12(gout, feat, acts, params, (hu, wu), m, cell_k=cell_k)
        torch.cuda.synchronize()
        err = float((df_a - df_b).abs().max())
        print(f"m{m} {(b, h, w, hu, wu)} d_feat {err:.3e} / {float(df_b.abs().max()):.3e}")
        assert err <= 5e-5 * float(df_b.abs().max())
        for name, x, y in zip(T.PARAM_NAMES, dp_a, dp_b):
            assert x.shape == y.shape, name
            err = float((x - y).abs().max())
            print(f"m{m} {(b, h, w, hu, wu)} {name} {err:.3e} / {float(y.abs().max()):.3e}")
            assert err <= 5e-5 * max(float(y.abs().max()), 1e-6), name


@pytest.mark.gpu
def test_cell_chain_bwd_kernel_alone():
    """diinn_cell_chain_bwd: random S, a chain workspace from diinn_cell_chain, random weights, against the recurrence
    g_3 = S_3, g_{i-1} = [k_{i-1} > 0] Kk_i^T g_i + S_{i-1} in float64.  B = 2, 5 x 7 (70 cells: a ragged last tile) and 1 x 1.
    Buffers are prefilled with NaN: the padding of S is not read as data, the padding of the tiled outputs and the guard zones
    around every output stay untouched; in place (dP_tiled = S) gives the same bits.
    Bound: three chained 256-term fp32 dot products against float64, 2e-5 of max|ref| (the plane chain's bound in test_training)."""
    import diinn_amd._native as N
    import diinn_amd.decoder as D
    import diinn_amd.training as T
    dev = torch.device("cuda:0")
    lib = N.load()
    gen = torch.Generator(device=dev).manual_seed(3)
    ptr = lambda x: C.c_void_p(x.data_ptr())                      # noqa: E731
    sd = synth.decoder_state_dict(9, 3.0, mode=2)
    packed = D.pack_state_dict(sd, mode=2).to(dev)
    kk = [None] + [torch.from_numpy(sd[f"K.{i}.0.weight"]).view(256, 832)[:, :256].double().to(dev) for i in (1, 2, 3)]
    nan = float("nan")
    guard = 1024
    for (b, h, w) in [(2, 5, 7), (1, 1, 1)]:
        cells = b * h * w
        tc = (cells + 31) // 32
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        chain = torch.randn((b, h, w, 1024), device=dev, generator=gen)
        N.check(lib.diinn_cell_chain(stream, ptr(chain), ptr(packed), b, h, w, 0, h), "cell_chain")
        s = torch.randn((1024, cells), device=dev, generator=gen)
        s_t = T.tile_planes(s)
        if cells % 32:
            s_t[-1, :, cells % 32:] = nan
        s_keep = s_t.clone()

        def guarded(numel):
            big = torch.full((numel + 2 * guard,), nan, device=dev)
            return big, big[guard:guard + numel]
        dp_big, dp = guarded(cells * 1024)
        dt_big, dt = guarded(tc * 1024 * 32)
        kt_big, kt = guarded(tc * 768 * 32)
        N.check(lib.diinn_cell_chain_bwd(stream, ptr(s_t), ptr(chain), ptr(packed), ptr(dp), ptr(dt), ptr(kt), b, h, w), "chain_bwd")
        torch.cuda.synchronize()
        same = lambda x, y: bool(((x == y) | (torch.isnan(x) & torch.isnan(y))).all())   # noqa: E731
        assert same(s_t, s_keep)                                                   # the input is not written
        for big in (dp_big, dt_big, kt_big):
            assert torch.isnan(big[:guard]).all() and torch.isnan(big[-guard:]).all()
        dt3, kt3 = dt.view(tc, 1024, 32), kt.view(tc, 768, 32)
        if cells % 32:
            assert torch.isnan(dt3[-1, :, cells % 32:]).all() and torch.isnan(kt3[-1, :, cells % 32:]).all()
        got = dp.view(b, 1024, h, w).permute(1, 0, 2, 3).reshape(1024, cells)
        assert torch.isfinite(got).all()
        assert torch.equal(T.untile_planes(dt3, cells), got)                       # both layouts hold the same values
        ck = chain.view(cells, 4, 256).permute(1, 2, 0)                            # slot i: k_i (slot 0: P_0)
        assert torch.equal(T.untile_planes(kt3, cells).view(3, 256, cells), torch.relu(ck[:3]))
        s64 = s.double().view(4, 256, cells)
        g = s64[3]
        ref = [None, None, None, g]
        for i in (3, 2, 1):
            g = (ck[i - 1] > 0) * (kk[i].t() @ g) + s64[i - 1]
            ref[i - 1] = g
        ref = torch.stack(ref)
        err = float((got.view(4, 256, cells).double() - ref).abs().max())
        print(f"cell_chain_bwd {(b, h, w)}: err {err:.3e} / max|ref| {float(ref.abs().max()):.3e}")
        assert err <= 2e-5 * float(ref.abs().max())
        # in place, without the k output
        dp2 = torch.full((cells * 1024,), nan, device=dev)
        N.check(lib.diinn_cell_chain_bwd(stream, ptr(s_t), ptr(chain), ptr(packed), ptr(dp2), ptr(s_t), None, b, h, w), "chain_bwd")
        torch.cuda.synchronize()
        assert torch.equal(dp2, dp) and same(s_t, dt3)
    assert lib.diinn_cell_chain_bwd(None, None, ptr(chain), ptr(packed), ptr(dp), ptr(dt), None, b, h, w) == N.ERR_INVALID_ARG
    assert lib.diinn_cell_chain_bwd(None, ptr(s_t), ptr(chain), ptr(packed), ptr(dp), None, None, b, h, w) == N.ERR_INVALID_ARG
    assert lib.diinn_cell_chain_bwd(None, ptr(s_t), ptr(chain), ptr(packed), ptr(dp), ptr(dt), None, 0, h, w) == N.ERR_INVALID_ARG
    assert lib.diinn_backward_data_qonly(None, ptr(s_t), ptr(s_t), ptr(packed), ptr(dt), ptr(dt), 0) == N.ERR_INVALID_ARG
    assert lib.diinn_decode_train_fwd_qonly(None, None, ptr(packed), ptr(dt), ptr(dt), 1, 1, 1, 2, 2, 2) == N.ERR_INVALID_ARG


@pytest.mark.gpu
@pytest.mark.parametrize("m", MODES)
def test_training_step_decreases_loss_modes12(m):
    """Six Adam steps of SRLitModule(arch="diinn", mode=m).step on the two-scale synthetic batch of
    test_training_step_decreases_loss: finite and decreasing loss."""
    import diinn_amd.modules as M
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    net = M.SRLitModule(arch="diinn", mode=m, init_q=False).to(dev).train()
    opt = torch.optim.Adam(net.parameters(), lr=1e-4)
    lr = torch.rand(2, 3, 16, 16, device=dev)
    batch = {2: (lr, torch.rand(2, 3, 32, 32, device=dev), ["a", "b"]),
             3: (lr, torch.rand(2, 3, 48, 48, device=dev), ["a", "b"])}
    losses = []
    for _ in range(6):
        opt.zero_grad(set_to_none=True)
        loss, _ = net.step(batch)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert all(np.isfinite(losses))
    assert losses[-1] < losses[0], losses


@pytest.mark.gpu
@pytest.mark.parametrize("m", MODES)
def test_backward_is_deterministic_modes12(m):
    """Two forward + backward passes on the same inputs give bit-identical outputs and gradients (no atomics anywhere)."""
    import diinn_amd.decoder as D
    dev = torch.device("cuda:0")
    sd, feat, r, (b, h, w, hu, wu) = _inputs("b2_12x10_31x27", m)
    dec = D.ImplicitDecoder(mode=m, init_q=False)
    dec.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    dec = dec.to(dev).train()
    rr = torch.from_numpy(r).to(dev)
    runs = []
    for _ in range(2):
        dec.zero_grad(set_to_none=True)
        x = torch.from_numpy(feat).to(dev).requires_grad_(True)
        y = dec(x, [hu, wu])
        (y * rr).sum().backward()
        torch.cuda.synchronize()
        runs.append([y.detach().clone(), x.grad.clone()] + [p.grad.clone() for p in dec.parameters()])
    for a, c in zip(*runs):
        assert torch.equal(a, c)
