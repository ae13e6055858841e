"""The callers' side of the boundary: DIINN / SRLitModule / RDN mirror."""
import json

import numpy as np
import pytest
import torch

import diinn_amd.synth as synth


def _shapes(golden, key):
    return json.loads(str(golden[key]))


def test_rdn_state_dict_matches_reference_and_output(golden):
    """Encoder stays PyTorch: same keys/shapes as reference rdn.py and the same output on CPU."""
    import diinn_amd.modules as M
    ref_shapes = _shapes(golden, "rdn/shapes_json")
    enc = M.make_rdn()
    assert {k: list(v.shape) for k, v in enc.state_dict().items()} == ref_shapes
    assert sum(p.numel() for p in enc.parameters()) == 21_973_952
    enc.load_state_dict({k: torch.from_numpy(v) for k, v in synth.state_dict_for(ref_shapes, 123, "enc.").items()})
    img = torch.from_numpy(synth.uniform(123, "img:1x3x12x10", (1, 3, 12, 10), 0.5) + np.float32(0.5))
    with torch.no_grad():
        out = enc.eval()(img).numpy()
    ref = golden["rdn/out_1x3x12x10"]
    assert float(np.abs(out - ref).max()) <= 1e-5 * max(1.0, float(np.abs(ref).max()))


def test_diinn_and_lit_module_key_names(golden):
    import diinn_amd.modules as M
    full = _shapes(golden, "diinn/shapes_json")
    net = M.DIINN(mode=3, init_q=False)
    assert {k: list(v.shape) for k, v in net.state_dict().items()} == full
    lit = M.SRLitModule(arch="diinn", mode=3, init_q=False)
    keys = set(lit.state_dict())
    assert {"net." + k for k in full} | {"sub", "div"} == keys          # sr_module.py:93-97
    assert lit.hparams.eval_bsize == 30000 and float(lit.sub) == 0.5


def test_load_from_checkpoint_roundtrip(tmp_path, golden):
    """A Lightning-style checkpoint dict (hyper_parameters + state_dict) loads by name."""
    import diinn_amd.modules as M
    full = _shapes(golden, "diinn/shapes_json")
    sd = {"net." + k: torch.from_numpy(v) for k, v in synth.state_dict_for(full, 123, "diinn.").items()}
    sd["sub"] = torch.full((1, 1, 1, 1), 0.5)
    sd["div"] = torch.full((1, 1, 1, 1), 0.5)
    path = tmp_path / "last.ckpt"
    torch.save({"state_dict": sd, "hyper_parameters": {"arch": "diinn", "mode": 3, "init_q": False, "lr": 1e-4,
                                                       "lr_gamma": 0.5, "lr_step": 10, "eval_bsize": 30000}}, path)
    lit = M.SRLitModule.load_from_checkpoint(str(path))
    assert lit.hparams.mode == 3 and not lit.training
    assert torch.equal(lit.net.decoder.K[1][0].weight, sd["net.decoder.K.1.0.weight"])


def test_bicubic_and_unknown_arch():
    import diinn_amd.modules as M
    y = M.SRLitModule(arch="bicubic")(torch.rand(1, 3, 8, 8), (16, 12))
    assert y.shape == (1, 3, 16, 12)
    assert isinstance(M.make_net("liif", 1, False), M.LIIF) and isinstance(M.make_net("metasr", 1, False), M.MetaSR)
    assert M.make_net("no-such-arch", 1, False) is None      # the reference's make_net falls through (sr_module.py:42-50)


@pytest.mark.gpu
def test_diinn_end_to_end_on_gpu_matches_reference(golden):
    """Encoder (PyTorch-ROCm) + HIP decoder vs the reference DIINN run on the CPU.  The encoder's
    GPU convolutions differ from the CPU's at ~1e-6; the tolerance is the decoder's 1e-4."""
    import diinn_amd.modules as M
    full = _shapes(golden, "diinn/shapes_json")
    dev = torch.device("cuda:0")
    net = M.DIINN(mode=3, init_q=False)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.state_dict_for(full, 123, "diinn.").items()})
    net = net.to(dev).eval()
    img = torch.from_numpy(synth.uniform(123, "img:1x3x12x10", (1, 3, 12, 10), 0.5) + np.float32(0.5)).to(dev)
    with torch.no_grad():
        out = net(img, [31, 27], 30000).cpu().numpy()
    ref = golden["diinn/out_1x3x12x10_to_31x27"]
    assert out.shape == ref.shape
    assert float(np.abs(out - ref).max()) <= 1e-4 * max(1.0, float(np.abs(ref).max()))


@pytest.mark.gpu
def test_lit_module_step_normalisation(golden):
    """SRLitModule.step: (x-.5)/.5 -> forward(.., hr.shape[-2:], eval_bsize) -> *.5+.5, clamp (sr_module.py:113-125)."""
    import diinn_amd.modules as M
    dev = torch.device("cuda:0")
    lit = M.SRLitModule(arch="diinn", mode=3, init_q=False).to(dev).eval()
    lr = torch.rand(1, 3, 10, 9, device=dev)
    hr = torch.rand(1, 3, 25, 22, device=dev)
    with torch.no_grad():
        loss, preds = lit.step({2.5: (lr, hr, "x")}, 30000)
        direct = lit((lr - 0.5) / 0.5, hr.shape[-2:], 30000)
    assert preds[2.5].shape == hr.shape and float(preds[2.5].min()) >= 0 and float(preds[2.5].max()) <= 1
    assert torch.allclose(preds[2.5], (direct * 0.5 + 0.5).clamp(0, 1))
    assert torch.isfinite(loss)


@pytest.mark.gpu
def test_graphed_forward_equals_eager():
    """hipGraph replay of encoder + decoder launches gives the eager result, also for new inputs."""
    import diinn_amd.modules as M
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    net = M.DIINN(mode=3, init_q=False).to(dev).eval()
    x1 = torch.rand(1, 3, 20, 24, device=dev)
    x2 = torch.rand(1, 3, 20, 24, device=dev)
    with torch.no_grad():
        e1, e2 = net(x1, (50, 61), 30000), net(x2, (50, 61), 30000)
        net.graphs = True
        g1 = net(x1, (50, 61), 30000)
        g2 = net(x2, (50, 61), 30000)
        g1b = net(x1, (50, 61), 30000)
    torch.cuda.synchronize()
    # MIOpen may pick another convolution algorithm under capture: rounding-level differences only
    assert torch.allclose(e1, g1, atol=1e-5) and torch.allclose(e2, g2, atol=1e-5)
    assert torch.allclose(g1, g1b, atol=1e-5) and not torch.allclose(g1, g2, atol=1e-5)
    assert len(net._graph_cache) == 1


@pytest.mark.gpu
def test_graph_replay_survives_larger_shape_and_knob_changes():
    """Replaying the graph of shape A after a LARGER shape B has run must not touch memory the caching
    allocator has handed to someone else (the P workspace of a capture lives in the graph's private pool),
    and changing a knob that selects other kernels (sine mode) must capture a new graph, not replay a stale one."""
    import diinn_amd._native as N
    import diinn_amd.modules as M
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    net = M.DIINN(mode=3, init_q=False, graphs=True).to(dev).eval()
    xa = torch.rand(1, 3, 16, 16, device=dev)
    xb = torch.rand(1, 3, 40, 40, device=dev)
    with torch.no_grad():
        net.graphs = False
        ea, eb = net(xa, (40, 40), 30000), net(xb, (100, 100), 30000)
        net.graphs = True
        ga = net(xa, (40, 40), 30000)          # captures A
        gb = net(xb, (100, 100), 30000)        # larger: the decoder's cached eager workspace is replaced
        held = gb.clone()
        # churn the allocator so a recycled block would be handed out again
        junk = [torch.full((n,), 7.0, device=dev) for n in (1 << 18, 1 << 20, 1 << 22)]
        ga2 = net(xa, (40, 40), 30000)         # replays A
        torch.cuda.synchronize()
        assert torch.allclose(ga, ea, atol=1e-5) and torch.allclose(ga2, ea, atol=1e-5)
        assert torch.allclose(gb, eb, atol=1e-5) and torch.equal(gb, held)
        assert all(bool((j == 7.0).all()) for j in junk)
        n_graphs = len(net._graph_cache)
        net.decoder.sin_mode = N.SIN_ACCURATE
        net(xa, (40, 40), 30000)
        assert len(net._graph_cache) == n_graphs + 1


def test_untrusted_checkpoint_is_refused_with_the_opt_in_named(tmp_path, monkeypatch):
    """A checkpoint that pickles a class outside torch's allow-list (what Lightning / LightningCLI runs can write) is
    not unpickled silently: the error names DIINN_TRUST_CKPT, and with the opt-in the same file loads."""
    import collections
    import diinn_amd.modules as M
    path = tmp_path / "cli.ckpt"
    lit = M.SRLitModule(arch="diinn", mode=3, init_q=False)
    torch.save({"state_dict": lit.state_dict(), "callbacks": collections.OrderedDict(a=_Opaque()),
                "hyper_parameters": {"arch": "diinn", "mode": 3, "init_q": False}}, str(path))
    monkeypatch.delenv("DIINN_TRUST_CKPT", raising=False)
    with pytest.raises(RuntimeError, match="DIINN_TRUST_CKPT=1"):
        M.SRLitModule.load_from_checkpoint(str(path))
    monkeypatch.setenv("DIINN_TRUST_CKPT", "1")
    again = M.SRLitModule.load_from_checkpoint(str(path))
    assert all(torch.equal(a, b) for a, b in zip(lit.state_dict().values(), again.state_dict().values()))


class _Opaque:
    """stands in for a Lightning callback state object"""
    x = 1


def test_set_split_bf16_switches_both_modes():
    import diinn_amd.modules as M
    net = M.DIINN(mode=3, init_q=False)
    assert net.decoder.compute == "f32" and net.encoder.hip_split_bf16 is False
    assert net.set_split_bf16() is net
    assert net.decoder.compute == "bf16x3" and net.encoder.hip_split_bf16 is True
    net.set_split_bf16(False)
    assert net.decoder.compute == "f32" and net.encoder.hip_split_bf16 is False


@pytest.mark.gpu
def test_rdn_weight_images_are_built_on_demand():
    """the derived weight images of the encoder are built only where a kernel reads them -- a map that runs
    F(4x4,3x3) layers never builds the F(2x2) image (diinn_rdn_forward_ex takes NULL for it there), a split-K map builds
    neither -- and free_unused_images() drops them without changing a result."""
    import diinn_amd._native as N
    import diinn_amd.modules as M
    dev = torch.device("cuda:0")
    torch.manual_seed(1)
    enc = M.make_rdn().to(dev).eval()
    lib = N.load()
    with torch.no_grad():
        small = torch.rand(1, 3, 24, 20, device=dev)
        a = enc(small)
        assert enc._hip_wu2 is None and enc._hip_wu4 is None     # split-K kernel: the 85 MB permutation image only
        big = torch.rand(1, 3, 200, 180, device=dev)
        assert lib.diinn_rdn_wino4_applies(1, 200, 180) == 1
        b = enc(big)
        assert enc._hip_wu4 is not None and enc._hip_wu2 is None
        mid = torch.rand(1, 3, 96, 100, device=dev)
        assert lib.diinn_rdn_wino4_applies(1, 96, 100) == 0
        c = enc(mid)
        assert enc._hip_wu2 is not None
        enc.free_unused_images(keep=("wino",))
        assert enc._hip_wu4 is None and enc._hip_wu2 is not None
        enc.free_unused_images()
        assert enc._hip_wu2 is None
        assert torch.equal(enc(small), a) and torch.equal(enc(big), b) and torch.equal(enc(mid), c)
