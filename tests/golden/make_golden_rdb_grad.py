#!/usr/bin/env python3
"""Gradient fixtures of one residual dense block (the encoder's training path: diinn_amd.encoder_training).

Runs only in the build container (needs /root/reference, read-only; never on the GPU box).

The reference's ``RDB(64, 64, 8)`` (src/models/components/rdn.py:19-35) under autograd, once in fp32 and once in float64, with
the synthetic per-layer-gain weights of the round-6 encoder fixtures (synth.state_dict_for(..., layer_gain_seed=...)): ``out`` and
the ``.grad`` of ``x`` and of all 18 parameter tensors under a seeded upstream gradient.  The tests rebuild the weights, the input
and the upstream gradient from synth (``case_inputs`` below is restated in tests/test_encoder_training.py), so a file stores
results only:

    out, d_x, the 9 bias gradients, d_W_LFF        in full (the float64 run; the weight gradient rounded to fp32 once)
    d_W_c of the 3x3 layers                         rows ``ROWS`` of every layer (the float64 run, rounded to fp32 once)
    dist/<tensor>, absmax/<tensor>                  max|fp32 run - float64 run| and max|float64 run| over the WHOLE tensor
    gates_open                                      fraction of open ReLU gates per layer (asserted in [0.25, 0.75] here)

Cases: B=2 at 12x10, B=1 at 7x5, B=1 at 1x1; one file per case.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_rdb_grad.py
"""
import os
import sys

os.environ.setdefault("PYTHONDONTWRITEBYTECODE", "1")
sys.dont_write_bytecode = True

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, "/root/reference")

import numpy as np  # noqa: E402
import torch  # noqa: E402

import diinn_amd.synth as synth  # noqa: E402
from src.models.components.rdn import RDB as RefRDB  # noqa: E402  (the reference)

CASES = [(2, 12, 10), (1, 7, 5), (1, 1, 1)]
GAIN_SEED = 91
ROWS = (5, 38)                      # output rows of every 3x3 weight gradient that a file keeps
NAMES = [f"convs.{c}.conv.0.{t}" for c in range(8) for t in ("weight", "bias")] + ["LFF.weight", "LFF.bias"]


def case_inputs(b, h, w):
    """(state dict, x, upstream gradient) of a case, all from synth."""
    shapes = {k: tuple(v.shape) for k, v in RefRDB(64, 64, 8).state_dict().items()}
    sd = synth.state_dict_for(shapes, 123, "rdb.", layer_gain_seed=GAIN_SEED)
    x = synth.normalish(11, f"rdb_x:{b}x{h}x{w}", (b, 64, h, w))
    r = synth.normalish(12, f"rdb_r:{b}x{h}x{w}", (b, 64, h, w))
    return sd, x, r


def run(sd, x, r, dtype):
    blk = RefRDB(64, 64, 8)
    blk.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    blk = blk.to(dtype)
    xt = torch.from_numpy(x).to(dtype).requires_grad_(True)
    gates = []
    hooks = [layer.conv[1].register_forward_hook(lambda m, i, o: gates.append(float((o > 0).double().mean()))) for layer in blk.convs]
    out = blk(xt)
    for hk in hooks:
        hk.remove()
    (out * torch.from_numpy(r).to(dtype)).sum().backward()
    named = dict(blk.named_parameters())
    res = {"out": out.detach(), "d_x": xt.grad}
    res.update({name: named[name].grad for name in NAMES})
    return {k: v.numpy() for k, v in res.items()}, gates


def main():
    for (b, h, w) in CASES:
        sd, x, r = case_inputs(b, h, w)
        r32, _ = run(sd, x, r, torch.float32)
        r64, gates = run(sd, x, r, torch.float64)
        print(f"B={b} {h}x{w}: gates open per layer " + " ".join(f"{g:.2f}" for g in gates))
        assert all(0.25 <= g <= 0.75 for g in gates), "a layer whose gates are (nearly) all open or all shut tests nothing of the gating"
        out = {"rows": np.array(ROWS, dtype=np.int64), "gates_open": np.array(gates), "gain_seed": np.int64(GAIN_SEED)}
        for name, v64 in r64.items():
            out[f"dist/{name}"] = np.float64(np.abs(r32[name].astype(np.float64) - v64).max())
            out[f"absmax/{name}"] = np.float64(np.abs(v64).max())
            if name.endswith(".weight") and name != "LFF.weight":
                out[f"ref/{name}"] = v64[list(ROWS)].astype(np.float32)
            elif name == "LFF.weight":
                out[f"ref/{name}"] = v64.astype(np.float32)
            else:
                out[f"ref/{name}"] = v64
        worst = max(NAMES + ["out", "d_x"], key=lambda n: out[f"dist/{n}"] / max(out[f"absmax/{n}"], 1e-300))
        print(f"   worst fp32-to-float64 distance relative to max|ref|: {worst} "
              f"{out['dist/' + worst] / out['absmax/' + worst]:.2e}")
        path = os.path.join(HERE, f"rdb_grad_b{b}_{h}x{w}.npz")
        np.savez(path, **out)
        print("   wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
