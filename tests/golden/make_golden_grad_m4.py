#!/usr/bin/env python3
"""Generate gradient fixtures for decoder mode 4 from the REAL reference decoder under autograd.

Build container only (needs /root/reference, read-only).  Runs the reference ``ImplicitDecoder(mode=4).forward(x, size, None)``
with autograd on -- the training path of sr_module.py:127-129; mode 4 is mode 3 with
``last_layer = Conv2d(256, 3, 3, padding=1, padding_mode='reflect')`` over the HR grid (diinn.py:89-90,140-147) -- for synthetic
weights/features regenerated from ``synth.py`` (``decoder_state_dict(seed, gain, mode=4)``, ``encoder_features``), with the scalar
loss  sum(out * R)  as in make_golden_grad.py (R from synth.py, so d loss / d out = R), in fp32 and once more in float64 (the same
module after ``.double()``: the truth).

Stored per case, in a file of its own (diinn_golden_grad_m4_<case>.npz, each below the 1 MiB a committed file may have):
  meta                      [b, h, w, hu, wu, gain, seed]
  out                       fp32 output
  grad/feat                 fp32 d loss / d features (whole)
  grad/<parameter>          fp32 d loss / d parameter; every weight with 256 output rows (the K and Q weights) at every
                            ROW_STRIDE-th output row (all columns), the biases and the 3x3 head [3,256,3,3] whole
  d64/<out|feat|parameter>  [max|fp32 - float64|, max|float64|] over the FULL tensor: the reference's own fp32 noise
Inputs are never stored.

Every case must keep the reference's own fp32 gradients within KEEP x max|float64| of its float64 run, per tensor: a tenth of the
project's gradient bound, so a ReLU gate that flips between the two precisions cannot eat the tests' margin.  A case that does not
stops the script (no case is skipped).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_grad_m4.py
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
from src.models.components.diinn import ImplicitDecoder  # noqa: E402  (the reference)

# (name, B, H, W, Hu, Wu, gain)
CASES = [
    ("c1x1_2x2", 1, 1, 1, 2, 2, 1.0),                   # the smallest output 'reflect' accepts: every tap is a border tap
    ("row3x2_2x7", 1, 3, 2, 2, 7, 1.0),                 # two rows: both row borders reflect into each other
    ("col4x3_9x2", 1, 4, 3, 9, 2, 1.0),                 # two columns
    ("b1_2x2_3x3", 1, 2, 2, 3, 3, 1.0),                 # one interior pixel
    ("b3_7x5_23x18", 3, 7, 5, 23, 18, 1.0),             # a batch: the reflection stays inside each image; ragged last tile
    ("b2_12x10_31x27_gain2", 2, 12, 10, 31, 27, 2.0),   # non-integer scale
    ("down16x12_8x6", 1, 16, 12, 8, 6, 1.0),            # down-scaling: most cells own no pixel
    ("b1_9x14_36x56_gain3", 1, 9, 14, 36, 56, 3.0),     # integer x4, stress weights
]
SEED = 123
ROW_STRIDE = 8
KEEP = 1e-5


def strided(pname):
    return pname[0] in "KQ" and pname.endswith("weight")


def run(sd, feat, r, size, dtype):
    dec = ImplicitDecoder(mode=4)
    dec.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    dec = dec.to(dtype).train()
    x = torch.from_numpy(feat).to(dtype).requires_grad_(True)
    y = dec(x, list(size), None)
    (y * torch.from_numpy(r).to(dtype)).sum().backward()
    grads = {pname: p.grad.numpy() for pname, p in dec.named_parameters()}
    return y.detach().numpy(), x.grad.numpy(), grads


def main():
    torch.manual_seed(0)
    for name, b, h, w, hu, wu, gain in CASES:
        out = {"meta": np.array([b, h, w, hu, wu, gain, SEED], dtype=np.float64)}
        sd = synth.decoder_state_dict(seed=SEED, gain=gain, mode=4)
        feat = synth.encoder_features(SEED, b, h, w)
        r = synth.uniform(SEED, f"gradw:m4:{name}", (b, 3, hu, wu), 1.0)
        y32, f32, g32 = run(sd, feat, r, (hu, wu), torch.float32)
        y64, f64, g64 = run(sd, feat, r, (hu, wu), torch.float64)

        def noise(a32, a64):
            return np.array([np.abs(a32.astype(np.float64) - a64).max(), np.abs(a64).max()], dtype=np.float64)

        out["out"] = y32.astype(np.float32)
        out["d64/out"] = noise(y32, y64)
        out["grad/feat"] = f32.astype(np.float32)
        out["d64/feat"] = noise(f32, f64)
        for pname, g in g32.items():
            out[f"d64/{pname}"] = noise(g, g64[pname])
            out[f"grad/{pname}"] = (g[::ROW_STRIDE] if strided(pname) else g).astype(np.float32)
        rel = {p: out[f"d64/{p}"][0] / max(out[f"d64/{p}"][1], 1e-30) for p in ["feat", *g32]}
        worst = max(rel, key=rel.get)
        print(name, "max|dfeat|=%.4f" % float(np.abs(f32).max()), "worst fp32-vs-f64 %.2e (%s)" % (rel[worst], worst))
        assert rel[worst] <= KEEP, (name, worst, rel[worst])
        path = os.path.join(HERE, f"diinn_golden_grad_m4_{name}.npz")
        np.savez_compressed(path, **out)
        print("wrote", path, os.path.getsize(path))
        assert os.path.getsize(path) < 900_000


if __name__ == "__main__":
    main()
