"""MetaSR in the hoisted form (opt-in ``MetaSR.hip_hoisted``): ``metasr_hoisted_kernel`` behind
``diinn_metasr_decode_hoisted`` and ``decoder.metasr_decode_hoisted``, in inference, under autograd and under graph replay.

CPU part: the switch, the header and the binding, argument validation without a device, the launches of the hoisted Function
(under the recorder's stubs), and the formula sheet ``metasr_forward_reference`` in fp32 on the ten reference cases.
GPU part: the ten cases against the reference outputs; the new kernel alone against a float64 evaluation of the same M under a
derived bound; written-once / row windows; plumbing; non-finite features; training against the reference's own gradients; graph
replay.

N of a case (test_metasr.py's definition) = the largest max|fp32 oracle - float64 oracle| over the fixture cases of the same gain."""
import contextlib
import ctypes as C
import importlib.util
import json
import os
import re
from unittest import mock

import numpy as np
import pytest
import torch

import diinn_amd.synth as synth
import metasr_oracle as MO

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PNAMES = ["layers.0.weight", "layers.0.bias", "layers.2.weight", "layers.2.bias"]
U = 2.0 ** -24                                                 # unit roundoff of fp32
WRITTEN_ONCE_SHAPES = [(3, 7, 5, 23, 18), (1, 1, 9, 4, 30), (2, 13, 3, 40, 9)]


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(HERE, "golden", "metasr_golden.npz"))


@pytest.fixture(scope="module")
def gold8():
    return np.load(os.path.join(HERE, "golden", "diinn_golden_r8.npz"))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    return torch.device("cuda:0")


def _imnet(gold, gain):
    shapes = {k: v for k, v in json.loads(str(gold["metasr/shapes_json"])).items() if k.startswith("imnet.")}
    return synth.state_dict_for(shapes, 123, "metasr.", gain=gain)


def _all_cases(gold, gold8):
    """(name, b, h, w, hu, wu, gain, reference output) of the 4 cases of metasr_golden.npz and the 6 metasr cases of r8."""
    out = []
    for k in gold.files:
        if k.startswith("meta/"):
            b, h, w, hu, wu, gain = gold[k]
            out.append((k[5:], int(b), int(h), int(w), int(hu), int(wu), float(gain), gold[f"out/{k[5:]}"]))
    for k in gold8.files:
        if k.startswith("out/metasr/"):
            name = k.split("/")[2]
            b, h, w, hu, wu, gain = gold8[f"meta/{name}"]
            out.append((name, int(b), int(h), int(w), int(hu), int(wu), float(gain), gold8[k]))
    return out


@pytest.fixture(scope="module")
def truth(gold, gold8):
    """({name: float64 oracle output}, {gain: N}) of the ten fixture cases, computed once."""
    o64, noise = {}, {}
    for name, b, h, w, hu, wu, gain, _ref in _all_cases(gold, gold8):
        sd, feat = _imnet(gold, gain), synth.encoder_features(123, b, h, w)
        o32 = MO.metasr_query_reference_form(sd, feat, (hu, wu)).numpy()
        o64[name] = MO.metasr_query_reference_form(sd, feat, (hu, wu), dtype=torch.float64).numpy()
        noise[gain] = max(noise.get(gain, 0.0), float(np.abs(o32 - o64[name]).max()))
    return o64, noise


def _params(sd, dev=None):
    ps = [torch.from_numpy(sd["imnet." + n]) for n in PNAMES]
    return ps if dev is None else [p.to(dev) for p in ps]


def _contract(ref):
    return 1e-4 * max(1.0, float(np.abs(ref).max()))


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------
def test_switch_defaults_keyword_and_graph_key():
    import diinn_amd.modules as M
    assert M.MetaSR.hip_hoisted is False
    net = M.make_net("metasr", 3, False)
    assert net.hip_hoisted is False and net.graphs is False
    on = M.MetaSR(hip_hoisted=True)
    assert on.hip_hoisted is True and M.MetaSR.hip_hoisted is False
    assert M.MetaSR(graphs=True, hip_hoisted=True).graphs is True
    x = torch.zeros(1, 3, 12, 10)
    off_key = net._graph_key(x, (31, 27))
    net.hip_hoisted = True
    on_key = net._graph_key(x, (31, 27))
    assert off_key != on_key
    net.hip_hoisted = False
    assert net._graph_key(x, (31, 27)) == off_key


def test_header_declares_and_binding_binds_the_entry_point():
    import diinn_amd._native as N
    header = open(os.path.join(ROOT, "include", "diinn_hip.h")).read()
    m = re.search(r"int\s+diinn_metasr_decode_hoisted\(([^)]*)\);", header)
    assert m, "include/diinn_hip.h does not declare diinn_metasr_decode_hoisted"
    args = [a.strip() for a in m.group(1).split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == ["stream", "M_dev", "packed_dev", "out_dev", "B", "H", "W", "Hu", "Wu", "y0", "y1"]
    res, argtypes = N.SIGNATURES["diinn_metasr_decode_hoisted"]
    assert res is C.c_int and argtypes == [C.c_void_p] * 4 + [C.c_int] * 7
    lib = N.load()
    assert lib.diinn_abi_version() == 11 and lib.diinn_metasr_decode_hoisted.argtypes == argtypes


def test_arguments_are_judged_before_the_launch():
    """On a machine without a GPU a launch would answer DIINN_ERR_HIP: INVALID_ARG / TOO_LARGE mean nothing was launched, and an
    empty window answers DIINN_OK without a launch."""
    import diinn_amd._native as N
    fn = N.load().diinn_metasr_decode_hoisted
    fake = C.c_void_p(4096)                                      # never dereferenced

    def call(m=fake, packed=fake, out=fake, b=1, h=8, w=8, hu=16, wu=16, y0=0, y1=16):
        return fn(None, m, packed, out, b, h, w, hu, wu, y0, y1)
    for null in ("m", "packed", "out"):
        assert call(**{null: None}) == N.ERR_INVALID_ARG
    for zero in ("b", "h", "w", "hu", "wu"):
        assert call(**{zero: 0, "y0": 0, "y1": 0}) == N.ERR_INVALID_ARG, zero
    assert call(hu=-3) == N.ERR_INVALID_ARG and call(w=-1) == N.ERR_INVALID_ARG
    assert call(y0=-1) == N.ERR_INVALID_ARG and call(y1=17) == N.ERR_INVALID_ARG
    assert call(y0=9, y1=3) == N.ERR_INVALID_ARG and call(y0=17, y1=17) == N.ERR_INVALID_ARG
    assert call(m=C.c_void_p(4100)) == N.ERR_INVALID_ARG         # the M rows are read 16 bytes at a time
    # more than 65,535 blocks of 16 rows in the window, a batch beyond the grid's z limit, an image of >= 2e9 pixels
    assert call(hu=16 * 65535 + 1, y1=16 * 65535 + 1) == N.ERR_TOO_LARGE
    assert call(b=65536) == N.ERR_TOO_LARGE
    assert call(hu=50000, wu=50000, y1=16) == N.ERR_TOO_LARGE
    for y in (0, 7, 16):
        assert call(y0=y, y1=y) == N.DIINN_OK                    # an empty window: nothing to do
    assert call(hu=16 * 65535 + 1, y0=5, y1=5) == N.DIINN_OK


def test_hoisted_function_launches_under_the_recorder():
    """The hoisted Function's forward is diinn_precompute_P_wpu then diinn_metasr_decode_hoisted -- never diinn_metasr_decode --
    and its backward is the default Function's, launch for launch (the recorder of tests/golden/make_training_launches.py)."""
    spec = importlib.util.spec_from_file_location("make_training_launches", os.path.join(HERE, "golden", "make_training_launches.py"))
    rec = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rec)
    MT = rec.MT
    log = []
    with rec.stubs(log):
        for shape in rec.SHAPES:
            b, h, w, hu, wu = shape
            hoisted = rec.run_case(MT.MetaSRHoistedFunction, (), MT.PARAM_NAMES, MT.PARAM_SHAPES, shape, True, (), log)
            direct = rec.run_case(MT.MetaSRFunction, (), MT.PARAM_NAMES, MT.PARAM_SHAPES, shape, True, (), log)
            assert hoisted[:2] == [["diinn_precompute_P_wpu", [b, h, w, 0, h]],
                                   ["diinn_metasr_decode_hoisted", [b, h, w, hu, wu, 0, hu]]]
            assert [c[0] for c in direct[:2]] == ["diinn_metasr_decode", "diinn_precompute_P_wpu"]
            assert hoisted[2:] == direct[2:] and len(hoisted) == len(direct)
            assert "diinn_metasr_decode" not in [c[0] for c in hoisted]


def test_formula_sheet_fp32_on_the_ten_reference_cases(gold, gold8, truth):
    """``metasr_forward_reference`` (the hoisted form in plain tensor algebra) in fp32 on the CPU: within 1e-4 x max(1, max|ref|)
    of the reference output on every case.  Measured here: 1.2e-6 .. 6.5e-5 against bounds of 1.6e-4 .. 7.3e-3, and 0.03 .. 0.45 N
    from the float64 oracle (N = 1.6e-5 at gain 1, 6.4e-5 at gain 2): the form is at least as accurate as the reference's."""
    import diinn_amd.metasr_training as MT
    o64, noise = truth
    cases = _all_cases(gold, gold8)
    assert len(cases) == 10
    geos = {c[1:6] for c in cases}
    assert {(1, 1, 1, 5, 7), (1, 1, 9, 4, 30), (1, 16, 12, 8, 6)} <= geos and (3, 7, 5, 23, 18) in geos
    assert any(c[1:6][1:] == (13, 3, 40, 9) for c in cases) and {c[6] for c in cases} == {1.0, 2.0}
    for name, b, h, w, hu, wu, gain, ref in cases:
        feat = torch.from_numpy(synth.encoder_features(123, b, h, w))
        out = MT.metasr_forward_reference(feat, _params(_imnet(gold, gain)), (hu, wu)).numpy()
        assert out.dtype == np.float32 and out.shape == ref.shape
        err32 = float(np.abs(out - ref).max())
        err64 = float(np.abs(out.astype(np.float64) - o64[name]).max())
        print(f"formula sheet {name}: max|sheet - ref32| = {err32:.3e} (bound {_contract(ref):.3e})  "
              f"max|sheet - f64| = {err64:.3e} = {err64 / noise[gain]:.2f} N (N = {noise[gain]:.3e})")
        assert err32 <= _contract(ref), f"{name}: {err32:.3e}"


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
def _decode(params, feat, size, dev, **kw):
    """``metasr_decode_hoisted`` on the images of ``params`` (tensors on ``dev``); feat a numpy array or a tensor."""
    import diinn_amd.decoder as D
    import diinn_amd.metasr_training as MT
    packed, image, _ = MT.images_on_device(params)
    if not isinstance(feat, torch.Tensor):
        feat = torch.from_numpy(feat).to(dev)
    return D.metasr_decode_hoisted(feat, packed, image, size, **kw)


@pytest.mark.gpu
def test_hoisted_decode_matches_reference_fixtures(gold, gold8, truth, dev):
    """The ten fixture cases through ``metasr_decode_hoisted``: within 1e-4 x max(1, max|ref|) of the reference output.  Recorded,
    not asserted (what the Winograd conv adds to M is part of it): the distance to the float64 oracle in units of N.
    Measured on the MI355X (N = 1.8e-5 at gain 1, 5.9e-5 at gain 2): against the reference 1.5e-6 (1x1 map) .. 8.4e-5 under bounds
    of 1.6e-4 .. 7.3e-3; against float64 gain 1 8.1e-7 .. 8.7e-6 = 0.05 .. 0.49 N, gain 2 3.4e-5 / 3.8e-5 = 0.57 / 0.65 N
    (metasr_kernel on the same cases: 0.05 .. 0.65 and 0.56 / 0.69 N)."""
    o64, noise = truth
    for name, b, h, w, hu, wu, gain, ref in _all_cases(gold, gold8):
        got = _decode(_params(_imnet(gold, gain), dev), synth.encoder_features(123, b, h, w), (hu, wu), dev).cpu().numpy()
        err32 = float(np.abs(got - ref).max())
        err64 = float(np.abs(got.astype(np.float64) - o64[name]).max())
        print(f"hoisted {name}: max|hip - ref32| = {err32:.3e} (bound {_contract(ref):.3e})  "
              f"max|hip - f64| = {err64:.3e} = {err64 / noise[gain]:.2f} N (N = {noise[gain]:.3e})")
        assert got.shape == ref.shape
        assert err32 <= _contract(ref), f"{name}: {err32:.3e}"


def _fuzz_geometries():
    """test_metasr.py's generator: twelve seeded geometries, B 1..3, H and W in 1..24, scales 0.5..5 each way, at most 20,000 HR
    pixels; the first two are forced to a 1-row and a 1-column map."""
    rng = np.random.default_rng(82)
    out = []
    while len(out) < 12:
        b, h, w = int(rng.integers(1, 4)), int(rng.integers(1, 25)), int(rng.integers(1, 25))
        if len(out) == 0:
            h = 1
        if len(out) == 1:
            w = 1
        hu = max(1, int(round(h * rng.uniform(0.5, 5.0))))
        wu = max(1, int(round(w * rng.uniform(0.5, 5.0))))
        if b * hu * wu <= 20000:
            out.append((b, h, w, hu, wu))
    return out


def _kernel_alone(params, feat, b, h, w, hu, wu, dev, tag):
    """The new kernel against sum_j h_j M_j + B0 in float64 from the M it read (h = relu(a) in float64), under the derived bound
        sum_j (eps_a,j |M_j| + g |h_j M_j|) + g |B0|,    g = 260 u (a 259-term fp32 sum),
        eps_a,j = 4 u (|w_r r_rev| + |w_w rel_w| + |w_h rel_h| + |b|)   (the three roundings of a; relu is 1-Lipschitz, so this
    also covers a mask that flips at the kink),   u = 2^-24.  Derived, not measured; measured on the MI355X: at most 0.017 of it."""
    import diinn_amd._native as N
    import diinn_amd.metasr_training as MT
    ws = torch.full((N.load().diinn_workspace_bytes(b, h, w) // 4,), float("nan"), device=dev)
    got = _decode(params, feat, (hu, wu), dev, workspace=ws)
    torch.cuda.synchronize()
    m = ws.view(b * h * w, 1024).double()
    assert bool(torch.isfinite(m[:, :771]).all())
    cell, inp = MT._pixel_tables(b, h, w, hu, wu, dev, torch.float64)      # the C ABI's fp32 tables, widened
    w1, b1 = params[0].double(), params[1].double()
    a = inp @ w1.t() + b1
    hid = torch.relu(a)
    eps_a = 4 * U * (inp.abs() @ w1.abs().t() + b1.abs())
    mc = m[cell][:, :768].view(-1, 3, 256)
    b0 = m[cell][:, 768:771]
    ref = torch.einsum("pj,pkj->pk", hid, mc) + b0
    g = 260 * U
    bound = torch.einsum("pj,pkj->pk", eps_a, mc.abs()) + g * torch.einsum("pj,pkj->pk", hid, mc.abs()) + g * b0.abs()
    err = (got.permute(0, 2, 3, 1).reshape(-1, 3).double() - ref).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"kernel alone {tag} {b}x{h}x{w}->{hu}x{wu}: max err {float(err.max()):.3e}, max err / bound {worst:.3f}")
    assert bool((err <= bound).all()), f"{tag}: err / bound up to {worst:.3f}"


@pytest.mark.gpu
def test_hoisted_kernel_alone_on_fixture_cases(gold, gold8, dev):
    for name, b, h, w, hu, wu, gain, _ref in _all_cases(gold, gold8):
        _kernel_alone(_params(_imnet(gold, gain), dev), synth.encoder_features(123, b, h, w), b, h, w, hu, wu, dev, name)


@pytest.mark.gpu
def test_hoisted_kernel_alone_on_fuzz_geometries(gold, dev):
    geos = _fuzz_geometries()
    assert sum(1 for g in geos if g[1] == 1 or g[2] == 1) >= 2
    assert any(g[3] < g[1] or g[4] < g[2] for g in geos)          # down-scaling: every lane its own cell, some cells unowned
    assert all(1 <= g[0] <= 3 and 1 <= g[1] <= 24 and 1 <= g[2] <= 24 and g[0] * g[3] * g[4] <= 20000 for g in geos)
    params = _params(_imnet(gold, 1.0), dev)
    for i, (b, h, w, hu, wu) in enumerate(geos):
        _kernel_alone(params, synth.encoder_features(200 + i, b, h, w), b, h, w, hu, wu, dev, f"fuzz {i}")


@pytest.mark.gpu
def test_hoisted_writes_every_output_once_and_row_windows(gold, dev):
    """``out`` prefilled with NaN is finite afterwards and equals the plain call; a NaN-prefilled workspace changes no bit; ``out=``
    is returned as given; ``rows=(y0, y1)`` writes those rows only (the rest keeps its NaN) and they are the full decode's rows bit
    for bit -- windows that start and end inside a 16-row block, a one-row window, and empty windows."""
    import diinn_amd._native as N
    params = _params(_imnet(gold, 1.0), dev)
    for (b, h, w, hu, wu) in WRITTEN_ONCE_SHAPES:
        feat = torch.from_numpy(synth.encoder_features(9, b, h, w)).to(dev)
        plain = _decode(params, feat, (hu, wu), dev)
        out = torch.full((b, 3, hu, wu), float("nan"), device=dev)
        ws = torch.full((N.load().diinn_workspace_bytes(b, h, w) // 4,), float("nan"), device=dev)
        ret = _decode(params, feat, (hu, wu), dev, out=out, workspace=ws)
        torch.cuda.synchronize()
        assert ret is out
        assert bool(torch.isfinite(out).all())
        assert torch.equal(out, plain)
        windows = [(0, 0), (hu, hu), (hu // 2, hu // 2), (0, 1), (hu - 1, hu), (1, hu - 1), (hu // 3, hu // 3 + 2)]
        if hu > 20:
            windows += [(3, 21), (5, 19), (17, 18), (16, hu), (0, 16)]
        for y0, y1 in windows:
            win = torch.full((b, 3, hu, wu), float("nan"), device=dev)
            assert _decode(params, feat, (hu, wu), dev, out=win, rows=(y0, y1)) is win
            torch.cuda.synchronize()
            assert torch.equal(win[:, :, y0:y1], plain[:, :, y0:y1]), (y0, y1)
            assert bool(torch.isnan(win[:, :, :y0]).all()) and bool(torch.isnan(win[:, :, y1:]).all()), (y0, y1)
        with pytest.raises(ValueError, match="rows must satisfy"):
            _decode(params, feat, (hu, wu), dev, rows=(2, hu + 1))
        with pytest.raises(ValueError, match="rows must satisfy"):
            _decode(params, feat, (hu, wu), dev, rows=(3, 2))


@pytest.mark.gpu
def test_hoisted_plumbing_determinism_side_stream_strided_input_and_out_validation(gold, dev):
    params = _params(_imnet(gold, 1.0), dev)
    b, h, w, hu, wu = 2, 9, 11, 21, 37
    feat = torch.from_numpy(synth.encoder_features(4, b, h, w)).to(dev)
    plain = _decode(params, feat, (hu, wu), dev)
    again = _decode(params, feat, (hu, wu), dev)
    torch.cuda.synchronize()
    assert torch.equal(plain, again)
    big = torch.zeros((b, 64, h + 3, 2 * w + 1), device=dev)
    view = big[:, :, 2:2 + h, 1:1 + 2 * w:2]
    view.copy_(feat)
    assert not view.is_contiguous()
    strided = _decode(params, view, (hu, wu), dev)
    torch.cuda.synchronize()
    assert torch.equal(strided, plain)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        on_side = _decode(params, feat, (hu, wu), dev)
    side.synchronize()
    assert torch.equal(on_side, plain)
    for bad in (torch.empty((b, 3, hu, wu + 1), device=dev), torch.empty((b, 3, wu, hu), device=dev).transpose(2, 3),
                torch.empty((b, 3, hu, wu), device=dev, dtype=torch.float64), torch.empty((b, 3, hu, wu))):
        with pytest.raises(ValueError, match="out must be a contiguous fp32"):
            _decode(params, feat, (hu, wu), dev, out=bad)
    with pytest.raises(RuntimeError, match="ROCm GPU"):
        _decode(params, feat.cpu(), (hu, wu), dev)


@pytest.mark.gpu
@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_hoisted_nonfinite_feature_value(gold, dev, bad):
    """One NaN / +Inf / -Inf feature value at a corner, an edge and in the interior of a 20 x 24 map (-> 66 x 80): every pixel the
    oracle marks non-finite is non-finite here; every pixel whose cell lies more than 6 cells from the value in either axis (the
    reach of a Winograd input tile) is finite and within the contract.  Nearer, the set may be larger than the oracle's: the conv's
    transforms mix the value into the tile's other cells."""
    import diinn_amd.decoder as D
    sd = _imnet(gold, 1.0)
    params = _params(sd, dev)
    iy = D.metasr_axis_tables(20, 66)[0].astype(np.int64)
    ix = D.metasr_axis_tables(24, 80)[0].astype(np.int64)
    for cy, cx in [(0, 23), (19, 9), (7, 9)]:
        feat = synth.encoder_features(11, 1, 20, 24).copy()
        feat[0, 17, cy, cx] = bad
        ref = MO.metasr_query_reference_form(sd, feat, (66, 80)).numpy()
        got = _decode(params, feat, (66, 80), dev).cpu().numpy()
        gn, rn = ~np.isfinite(got), ~np.isfinite(ref)
        assert rn.any() and not rn.all(), (bad, cy, cx)
        assert bool(gn[rn].all()), f"{bad} at ({cy},{cx}): {int((rn & ~gn).sum())} of the oracle's non-finite values are finite here"
        far = (np.abs(iy - cy) > 6)[:, None] | (np.abs(ix - cx) > 6)[None, :]
        far = np.broadcast_to(far, got.shape)
        assert far.any() and not rn[far].any()
        assert not gn[far].any(), f"{bad} at ({cy},{cx}): {int(gn[far].sum())} non-finite values more than 6 cells away"
        assert float(np.abs(got[far] - ref[far]).max()) <= _contract(ref[far]), (bad, cy, cx)
        print(f"non-finite {bad} at ({cy},{cx}): oracle {int(rn.sum())} values, hoisted {int(gn.sum())}")


# ---- training ----------------------------------------------------------------------------------
GRAD_CASES = ["b2_12x10_31x27", "b1_9x14_36x56_gain2", "b1_8x8_5x6_down", "b1_1x1_7x5"]
GRAD_SHAPES = {"imnet.layers.0.weight": (256, 3), "imnet.layers.0.bias": (256,),
               "imnet.layers.2.weight": (1728, 256), "imnet.layers.2.bias": (1728,)}
ROW_STRIDE = 8
RTOL = 1e-4                      # the project's gradient bound: max|g - ref| <= 1e-4 max|ref| per tensor


def _grad_inputs(name):
    g = np.load(os.path.join(HERE, "golden", f"metasr_golden_grad_{name}.npz"))
    b, h, w, hu, wu, gain, seed = g["meta"]
    b, h, w, hu, wu, seed = int(b), int(h), int(w), int(hu), int(wu), int(seed)
    sd = synth.state_dict_for(GRAD_SHAPES, seed, "metasr.", gain=float(gain))
    r = synth.uniform(seed, f"gradw:metasr:{name}", (b, 3, hu, wu), 1.0)
    return g, [sd["imnet." + n] for n in PNAMES], synth.encoder_features(seed, b, h, w), r, (b, h, w, hu, wu)


class _GivenFeatures(torch.nn.Module):
    """Stands in for the encoder: returns the given feature map (a leaf that requires grad)."""

    out_dim = 64

    def __init__(self, feat):
        super().__init__()
        self.feat = feat

    def forward(self, inp):
        return self.feat


@contextlib.contextmanager
def _counted_launches(counts):
    """Every call of a stream-taking entry point on the loaded library is counted by name and passed on."""
    import diinn_amd._native as N
    lib = N.load()

    class Proxy:
        def __getattr__(self, name):
            fn = getattr(lib, name)
            if name not in N.SIGNATURES or N.SIGNATURES[name][1][:1] != [C.c_void_p]:
                return fn

            def launch(*args):
                counts[name] = counts.get(name, 0) + 1
                return fn(*args)
            return launch
    with mock.patch.object(N, "load", lambda: Proxy()):
        yield


@pytest.mark.gpu
@pytest.mark.parametrize("name", GRAD_CASES)
def test_hoisted_autograd_against_reference_fixtures(name):
    """``MetaSR(hip_hoisted=True)`` under autograd on given features: the output is the no_grad hoisted output bit for bit and within
    1e-4 x max(1, max|ref|) of the reference's; every gradient within 1e-4 x max|ref| of the reference's own .grad
    (layers.2.weight: every 8th row is pinned).  The forward launches the conv and the new kernel, never diinn_metasr_decode."""
    import diinn_amd.modules as M
    dev = torch.device("cuda:0")
    g, ws, feat, r, (b, h, w, hu, wu) = _grad_inputs(name)
    net = M.MetaSR(hip_hoisted=True)
    net.imnet.load_state_dict({n: torch.from_numpy(x) for n, x in zip(PNAMES, ws)}, strict=True)
    net = net.to(dev).train()
    x = torch.from_numpy(feat).to(dev).requires_grad_(True)
    net.encoder = _GivenFeatures(x)
    inp = torch.zeros((b, 3, h, w), device=dev)
    counts = {}
    with _counted_launches(counts):
        y = net(inp, (hu, wu))
    assert counts == {"diinn_precompute_P_wpu": 1, "diinn_metasr_decode_hoisted": 1}, counts
    assert y.requires_grad
    counts = {}
    with torch.no_grad(), _counted_launches(counts):
        y0 = net(inp, (hu, wu))
    assert counts == {"diinn_precompute_P_wpu": 1, "diinn_metasr_decode_hoisted": 1}, counts
    assert torch.equal(y.detach(), y0)
    yb = net(inp, (hu, wu), 300)                                  # bsize: the reference's no_grad decode
    assert not yb.requires_grad and torch.equal(yb, y0)
    ref_out = g["out"]
    err = float(np.abs(y0.cpu().numpy() - ref_out).max())
    print(f"{name} hoisted out: err {err:.3e} (bound {_contract(ref_out):.3e})")
    assert err <= _contract(ref_out)
    net.hip_hoisted = False                                       # the switch is read per call: the default path is metasr_kernel's
    counts = {}
    with torch.no_grad(), _counted_launches(counts):
        yd = net(inp, (hu, wu))
    assert counts == {"diinn_metasr_decode": 1}, counts
    assert float((yd - y0).abs().max()) <= 2 * _contract(ref_out)
    (y * torch.from_numpy(r).to(dev)).sum().backward()
    named = dict(net.imnet.named_parameters())
    for pname, got in [("feat", x.grad)] + [(n, named[n].grad) for n in PNAMES]:
        ref = g[f"grad/{pname}"]
        got = got.cpu().numpy()
        if pname == "layers.2.weight":
            got = got[::ROW_STRIDE]
        assert got.shape == ref.shape, (pname, got.shape, ref.shape)
        e = float(np.abs(got.astype(np.float64) - ref).max())
        bound = RTOL * max(float(np.abs(ref).max()), 1e-6)
        print(f"{name} hoisted {pname}: err {e:.3e} / max|ref| {float(np.abs(ref).max()):.3e} (bound {bound:.3e})")
        assert e <= bound, f"{name} {pname} err {e:.3e} > {bound:.3e}"


@pytest.mark.gpu
def test_hoisted_backward_is_deterministic_and_honours_needs_input_grad():
    """The rule of test_metasr_training.py on the hoisted Function: two passes are bit-identical; a subset of inputs requiring grad
    returns exactly that subset, with the values of the full pass -- which are the default Function's (the same backward on the
    same M)."""
    import diinn_amd.metasr_training as MT
    dev = torch.device("cuda:0")
    _g, ws, feat, r, (b, h, w, hu, wu) = _grad_inputs("b2_12x10_31x27")
    rr = torch.from_numpy(r).to(dev)

    def run(feat_grad, which, fn=MT.MetaSRHoistedFunction):
        params = [torch.from_numpy(x).to(dev).requires_grad_(n in which) for n, x in zip(PNAMES, ws)]
        x = torch.from_numpy(feat).to(dev).requires_grad_(feat_grad)
        y = fn.apply(x, hu, wu, *params)
        (y * rr).sum().backward()
        return y.detach(), x.grad, [p.grad for p in params]

    y1, f1, g1 = run(True, PNAMES)
    y2, f2, g2 = run(True, PNAMES)
    assert torch.equal(y1, y2) and torch.equal(f1, f2) and all(torch.equal(a, c) for a, c in zip(g1, g2))
    _, f0, g0 = run(True, PNAMES, MT.MetaSRFunction)
    assert torch.equal(f0, f1) and all(torch.equal(a, c) for a, c in zip(g0, g1))
    _, f3, g3 = run(True, [])
    assert torch.equal(f3, f1) and all(g is None for g in g3)
    _, f4, g4 = run(False, ["layers.0.bias", "layers.2.weight"])
    assert f4 is None and g4[0] is None and g4[3] is None
    assert torch.equal(g4[1], g1[1]) and torch.equal(g4[2], g1[2])
    _, f5, g5 = run(False, ["layers.0.weight"])
    assert f5 is None and torch.equal(g5[0], g1[0]) and g5[1] is None and g5[2] is None and g5[3] is None


@pytest.mark.gpu
def test_srlitmodule_metasr_hoisted_training_steps():
    """Two Adam steps of SRLitModule(arch="metasr") with the switch on, on a 12x10 batch: finite loss, the parameters move, and
    diinn_metasr_decode is never launched."""
    import diinn_amd.modules as M
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    net = M.SRLitModule(arch="metasr").to(dev).train()
    net.net.hip_hoisted = True
    opt = torch.optim.Adam(net.parameters(), lr=1e-4)
    lr = torch.rand(2, 3, 12, 10, device=dev)
    batch = {2: (lr, torch.rand(2, 3, 24, 20, device=dev), ["a", "b"]),
             3: (lr, torch.rand(2, 3, 31, 27, device=dev), ["a", "b"])}
    before = [p.detach().clone() for p in net.net.imnet.parameters()]
    counts, losses = {}, []
    with _counted_launches(counts):
        for _ in range(2):
            opt.zero_grad(set_to_none=True)
            loss, _ = net.step(batch)
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
    assert all(np.isfinite(losses)), losses
    assert all(not torch.equal(p.detach(), q) for p, q in zip(net.net.imnet.parameters(), before))
    assert counts.get("diinn_metasr_decode_hoisted") == 4 and "diinn_metasr_decode" not in counts, counts


# ---- graph replay ------------------------------------------------------------------------------
@pytest.mark.gpu
def test_hoisted_graph_replay(gold):
    """MetaSR(graphs=True, hip_hoisted=True) at 1x3x12x10 -> 31x27: the replayed output is the eager hoisted output bit for bit,
    twice (the second call replays); an in-place change of imnet.layers.2.weight captures anew and changes the output; the first
    graph's entry still holds the images it was captured on."""
    import diinn_amd.modules as M
    dev = torch.device("cuda:0")
    full = json.loads(str(gold["metasr/shapes_json"]))
    state = {k: torch.from_numpy(v) for k, v in synth.state_dict_for(full, 123, "metasrnet.").items()}
    eager = M.MetaSR(hip_hoisted=True)
    eager.load_state_dict(state)
    eager = eager.to(dev).eval()
    net = M.MetaSR(graphs=True, hip_hoisted=True)
    net.load_state_dict(state)
    net = net.to(dev).eval()
    img = torch.from_numpy(synth.uniform(123, "img:1x3x12x10", (1, 3, 12, 10), 0.5) + np.float32(0.5)).to(dev)
    with torch.no_grad():
        want = eager(img, [31, 27])
        g1 = net(img, [31, 27])
        g2 = net(img, [31, 27])
        torch.cuda.synchronize()
        assert len(net._graph_cache) == 1
        assert torch.equal(g1, want) and torch.equal(g2, want)
        ref = gold["metasr/out_1x3x12x10_to_31x27"]
        assert float(np.abs(want.cpu().numpy() - ref).max()) <= 2e-4 * max(1.0, float(np.abs(ref).max()))
        kept = next(iter(net._graph_cache.values()))[3]
        first = net._hoisted_images
        assert len(first) == 3 and any(k is first for k in kept)
        dict(net.imnet.named_parameters())["layers.2.weight"].mul_(1.5)
        dict(eager.imnet.named_parameters())["layers.2.weight"].mul_(1.5)
        g3 = net(img, [31, 27])
        torch.cuda.synchronize()
        assert len(net._graph_cache) == 2
        assert not torch.equal(g3, g1) and torch.equal(g3, eager(img, [31, 27]))
        assert net._hoisted_images[0] is not first[0]             # new images; the first entry keeps its own
        assert next(iter(net._graph_cache.values()))[3] is kept and any(k is first for k in kept)
