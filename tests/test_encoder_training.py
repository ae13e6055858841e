"""CPU tests of the encoder's training path (diinn_amd.encoder_training; GPU tests: test_encoder_training_gpu.py).

Fixtures: tests/golden/rdb_grad_*.npz (make_golden_rdb_grad.py: the reference's RDB under autograd, fp32 and float64).
Bounds per tensor, against the float64 run:
    contract   1e-4 x max|ref grad| (the project's gradient contract);
    floor      3 x the reference's own fp32-to-float64 distance on that tensor + 2^-23 x max|ref| -- the noise floor: the stored
               float64 value rounded to fp32 once (2^-24) and the result's own rounding to fp32 (2^-24).
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import diinn_amd._native as N
import diinn_amd.encoder_training as ET
import diinn_amd.modules as M
import diinn_amd.synth as synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = [(2, 12, 10), (1, 7, 5), (1, 1, 1)]
NAMES = [f"convs.{c}.conv.0.{t}" for c in range(8) for t in ("weight", "bias")] + ["LFF.weight", "LFF.bias"]
FLOOR = 2.0 ** -23


def load_case(b, h, w):
    return np.load(os.path.join(GOLDEN, f"rdb_grad_b{b}_{h}x{w}.npz"))


def case_inputs(b, h, w, gain_seed):
    """make_golden_rdb_grad.case_inputs restated: (state dict, x, upstream gradient), bit-identical to the generator's."""
    shapes = {k: tuple(v.shape) for k, v in M.RDB(64, 64, 8).state_dict().items()}
    sd = synth.state_dict_for(shapes, 123, "rdb.", layer_gain_seed=gain_seed)
    x = synth.normalish(11, f"rdb_x:{b}x{h}x{w}", (b, 64, h, w))
    r = synth.normalish(12, f"rdb_r:{b}x{h}x{w}", (b, 64, h, w))
    return sd, x, r


def check_against_fixture(gold, got, what, contract_only=False):
    """got: {"out", "d_x", parameter names} -> arrays.  Prints every figure, then asserts both bounds (module docstring)."""
    rows = [int(r) for r in gold["rows"]]
    bad = []
    for name in ["d_x"] + NAMES:
        ref = gold[f"ref/{name}"].astype(np.float64)
        g = np.asarray(got[name], dtype=np.float64)
        if name.endswith(".weight") and name != "LFF.weight":
            g = g[rows]
        assert g.shape == ref.shape, (name, g.shape, ref.shape)
        err = float(np.abs(g - ref).max())
        amax, dist = float(gold[f"absmax/{name}"]), float(gold[f"dist/{name}"])
        contract, floor = 1e-4 * amax, 3 * dist + FLOOR * amax
        print(f"{what} {name}: err {err:.3e}  contract {contract:.3e}  3 x dist + floor {floor:.3e}  (dist {dist:.3e}, max|ref| {amax:.3e})")
        if err > contract or (not contract_only and err > floor):
            bad.append((name, err, contract, floor))
    assert not bad, f"{what}: {bad}"


def dense_buffer(params, x):
    buf = x.new_empty((x.shape[0], 576, x.shape[2], x.shape[3]))
    buf[:, :64] = x
    for c in range(8):
        cin = 64 * (c + 1)
        buf[:, cin:cin + 64] = F.relu(F.conv2d(buf[:, :cin], params[2 * c], params[2 * c + 1], padding=1))
    return buf


@pytest.mark.parametrize("b,h,w", CASES)
def test_rdb_backward_reference_against_fixtures(b, h, w):
    gold = load_case(b, h, w)
    assert all(0.25 <= g <= 0.75 for g in gold["gates_open"])
    sd, x, r = case_inputs(b, h, w, int(gold["gain_seed"]))
    params = [torch.from_numpy(sd[n]) for n in NAMES]
    xt, rt = torch.from_numpy(x), torch.from_numpy(r)
    buf = dense_buffer(params, xt)
    out = F.conv2d(buf, params[16], params[17]) + xt
    ref_out = gold["ref/out"]
    assert float(np.abs(out.numpy() - ref_out).max()) <= 3 * float(gold["dist/out"]) + FLOOR * float(gold["absmax/out"])
    d_x, grads = ET.rdb_backward_reference(rt, buf, params)
    got = {"d_x": d_x.numpy(), **{n: g.numpy() for n, g in zip(NAMES, grads)}}
    check_against_fixture(gold, got, f"reference B={b} {h}x{w}")


@pytest.mark.parametrize("j", [0, 3, 7])
def test_transposed_weight_builder(j):
    """conv3x3(G[:, 64j:]; Wt_j) is the sum over the layers c >= j of layer c's input gradient at group j (float64)."""
    gen = torch.Generator().manual_seed(5 + j)
    ws = [torch.randn(64, 64 * (c + 1), 3, 3, dtype=torch.float64, generator=gen) for c in range(8)]
    g = torch.randn(1, 512, 5, 4, dtype=torch.float64, generator=gen)
    wt = ET.transposed_weight(ws, j)
    assert tuple(wt.shape) == (64, 64 * (8 - j), 3, 3)
    got = F.conv2d(g[:, 64 * j:], wt, padding=1)
    ref = sum(torch.nn.grad.conv2d_input((1, 64 * (c + 1), 5, 4), ws[c], g[:, 64 * c:64 * c + 64], padding=1)[:, 64 * j:64 * j + 64]
              for c in range(j, 8))
    assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
    with pytest.raises(ValueError):
        ET.transposed_weight(ws, 8)


def test_symbols_bound_and_bad_arguments_return_a_status():
    lib = N.load()
    assert N.ABI_VERSION == 11 and lib.diinn_abi_version() == 11
    for name in ("diinn_relu_gate", "diinn_conv_wgrad"):
        assert name in N.SIGNATURES and getattr(lib, name).argtypes is not None
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "diinn_hip.h")).read()
    assert "int diinn_relu_gate(" in header and "int diinn_conv_wgrad(" in header and "rdn.py:15-17" in header and "rdn.py:34-35" in header
    p = C.c_void_p(0x10000)                                      # never dereferenced: every call below fails its checks first
    ok = dict(g=p, gbs=64, x=p, xbs=64, cin=64, taps=9, part=p, nsplit=1, b=1, h=1, w=1)

    def wgrad(**kw):
        a = {**ok, **kw}
        return lib.diinn_conv_wgrad(None, a["g"], a["gbs"], a["x"], a["xbs"], a["cin"], a["taps"], a["part"], a["nsplit"], a["b"], a["h"], a["w"])

    for bad in (dict(g=None), dict(x=None), dict(part=None), dict(cin=96), dict(cin=640), dict(cin=0), dict(taps=4), dict(nsplit=0),
                dict(b=0), dict(h=-1), dict(g=C.c_void_p(0x10002)), dict(gbs=-1)):
        assert wgrad(**bad) != N.DIINN_OK, bad
    gate = lambda d, y, g, b=1, h=1, w=1, bs=64: lib.diinn_relu_gate(None, d, bs, y, bs, g, bs, b, h, w)   # noqa: E731
    assert gate(None, p, p) != N.DIINN_OK and gate(p, None, p) != N.DIINN_OK and gate(p, p, None) != N.DIINN_OK
    assert gate(p, p, p, b=0) != N.DIINN_OK and gate(p, p, p, w=0) != N.DIINN_OK
    assert gate(p, p, p, b=2, bs=63) != N.DIINN_OK                # images would overlap
    assert gate(C.c_void_p(0x10001), p, p) != N.DIINN_OK


def test_flag_defaults_off_and_cpu_training_is_unchanged():
    assert M.RDN.hip_autograd is False and M.RDN().hip_autograd is False
    assert M.DIINN(mode=3, init_q=False).encoder.hip_autograd is False
    torch.manual_seed(3)
    rdb = M.RDB(64, 64, 8)
    x = torch.randn(1, 64, 6, 5)

    def grads(fn):
        rdb.zero_grad(set_to_none=True)
        xi = x.clone().requires_grad_(True)
        fn(xi).sum().backward()
        return [xi.grad] + [p.grad.clone() for p in rdb.parameters()]

    before = grads(lambda t: rdb.LFF(rdb.convs(t)) + t)          # RDB.forward as it was
    for got in (grads(rdb), grads(lambda t: rdb(t, True, 1 << 20))):      # ... as it is; and with the flag on a CPU tensor
        assert all(torch.equal(a, b) for a, b in zip(before, got))
    assert ET.block_applies(rdb) and not ET.block_applies(M.RDB(32, 32, 6))
    enc = M.RDN()
    img = torch.rand(1, 3, 6, 5)
    enc.zero_grad()
    enc(img).sum().backward()
    off = [p.grad.clone() for p in enc.parameters()]
    enc.hip_autograd = True                                      # CPU input: today's path
    enc.zero_grad()
    enc(img).sum().backward()
    assert all(torch.equal(a, p.grad) for a, p in zip(off, enc.parameters()))
    with pytest.raises(NotImplementedError):
        ET.RDBFunction.apply(x, *ET.block_params(rdb))           # no CPU form, no fallback
