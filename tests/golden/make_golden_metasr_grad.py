#!/usr/bin/env python3
"""Generate gradient fixtures for the MetaSR comparison decoder from the REAL reference under autograd.

Build container only (needs /root/reference, read-only).  Runs the reference ``MetaSR.query_rgb``
(src/models/components/metasr.py:70-104) on given features with autograd on -- the decoder's part of the training path
sr_module.py:127-129 -> forward(lr, size, None) -- for synthetic ``imnet`` weights / features regenerated from ``synth.py``,
with the scalar loss  sum(out * R)  (R from synth.py, so d loss / d out = R), in fp32 and once more in float64.

float64: the reference MetaSR does not run in float64 as it is (``make_coord`` ends in ``.float()`` and grid_sample rejects
the dtype mix), so ``make_coord`` is wrapped ON THE INSTANCE to cast its result to double; with that the ``.double()``
module runs.

The ReLU kink: the HIP kernel's fmaf order differs from ATen's, so a pre-activation ``a`` of imnet.layers.0 within a few ulp
of 0 could flip a mask.  ``a`` is taken with a forward hook; seeds are tried from 123 upwards and the first with
min|a| >= 2e-6 * gain is kept (asserted; seed and minimum are stored).  A condition on the inputs, not a tolerance.

Stored per case, in a file of its own (metasr_golden_grad_<case>.npz, each below 1 MiB):
  meta                      [b, h, w, hu, wu, gain, seed]
  min_abs_a                 min|a| over every pixel and hidden channel
  out                       fp32 output
  grad/feat                 fp32 d loss / d features
  grad/<imnet parameter>    fp32 d loss / d parameter; layers.2.weight at every 8th row (all columns)
  d64/<out|feat|parameter>  [max|fp32 - float64|, max|float64|] over the FULL tensor: the reference's own fp32 noise
Inputs are never stored.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_metasr_grad.py
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
from src.models.components.metasr import MetaSR  # noqa: E402  (the reference)

# (name, B, H, W, Hu, Wu, gain)
CASES = [
    ("b2_12x10_31x27", 2, 12, 10, 31, 27, 1.0),          # non-integer scale, different per axis: 240 cells = 7.5 plane tiles
    ("b1_9x14_36x56_gain2", 1, 9, 14, 36, 56, 2.0),      # exact x4: every pixel's left edge on a cell boundary (the +1e-6 decides)
    ("b1_8x8_5x6_down", 1, 8, 8, 5, 6, 1.0),             # down-scaling: most cells own no pixel
    ("b1_1x1_7x5", 1, 1, 1, 7, 5, 1.0),                  # one cell
]
ROW_STRIDE = 8
FIRST_SEED = 123
MIN_ABS_A = 2e-6                                         # x gain
IMNET_SHAPES = {"imnet.layers.0.weight": (256, 3), "imnet.layers.0.bias": (256,),
                "imnet.layers.2.weight": (1728, 256), "imnet.layers.2.bias": (1728,)}


def inputs(seed, name, b, h, w, hu, wu, gain):
    sd = synth.state_dict_for(IMNET_SHAPES, seed, "metasr.", gain=gain)
    feat = synth.encoder_features(seed, b, h, w)
    r = synth.uniform(seed, f"gradw:metasr:{name}", (b, 3, hu, wu), 1.0)
    return sd, feat, r


def run(model, sd, feat, r, size, dtype):
    model.load_state_dict({k: torch.from_numpy(v).to(dtype) for k, v in sd.items()}, strict=False)
    model.zero_grad(set_to_none=True)
    seen = []
    hook = model.imnet.layers[0].register_forward_hook(lambda mod, args, res: seen.append(res.detach()))
    x = torch.from_numpy(feat).to(dtype).requires_grad_(True)
    coord, cell = model.make_coord_and_cell(x, size)
    y = model.reshape_pred(model.query_rgb(x, coord, cell), size)
    hook.remove()
    (y * torch.from_numpy(r).to(dtype)).sum().backward()
    grads = {k[len("imnet."):]: p.grad.numpy() for k, p in model.named_parameters() if k.startswith("imnet.")}
    return y.detach().numpy(), x.grad.numpy(), grads, float(seen[0].abs().min())


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    m32 = MetaSR().train()
    m64 = MetaSR().double().train()
    make_coord = m64.make_coord
    m64.make_coord = lambda *a, **k: make_coord(*a, **k).double()
    for name, b, h, w, hu, wu, gain in CASES:
        seed = FIRST_SEED
        while True:
            sd, feat, r = inputs(seed, name, b, h, w, hu, wu, gain)
            y32, f32, g32, min_a = run(m32, sd, feat, r, (hu, wu), torch.float32)
            if min_a >= MIN_ABS_A * gain:
                break
            print(name, "seed", seed, "min|a| = %.3e: next seed" % min_a)
            seed += 1
        assert min_a >= MIN_ABS_A * gain
        y64, f64, g64, _ = run(m64, sd, feat, r, (hu, wu), torch.float64)
        assert y64.dtype == np.float64 and f64.dtype == np.float64

        def noise(a32, a64):
            return np.array([np.abs(a32.astype(np.float64) - a64).max(), np.abs(a64).max()], dtype=np.float64)

        out = {"meta": np.array([b, h, w, hu, wu, gain, seed], dtype=np.float64), "min_abs_a": np.array(min_a, dtype=np.float64),
               "out": y32.astype(np.float32), "d64/out": noise(y32, y64),
               "grad/feat": f32.astype(np.float32), "d64/feat": noise(f32, f64)}
        for pname, g in g32.items():
            out[f"d64/{pname}"] = noise(g, g64[pname])
            out[f"grad/{pname}"] = (g[::ROW_STRIDE] if pname == "layers.2.weight" else g).astype(np.float32)
        worst = max(out[f"d64/{p}"][0] / max(out[f"d64/{p}"][1], 1e-30) for p in list(g32) + ["feat"])
        print(name, "seed", seed, "min|a| = %.3e" % min_a, "max|dfeat|=%.4f" % float(np.abs(f32).max()), "worst fp32-vs-f64 %.2e" % worst)
        path = os.path.join(HERE, f"metasr_golden_grad_{name}.npz")
        np.savez_compressed(path, **out)
        print("wrote", path, os.path.getsize(path))


if __name__ == "__main__":
    main()
