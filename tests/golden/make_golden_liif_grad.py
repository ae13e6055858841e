#!/usr/bin/env python3
"""Generate gradient fixtures for the LIIF comparison decoder from the REAL reference under autograd.

Build container only (needs /root/reference, read-only).  Runs the reference ``LIIF.query_rgb`` + ``reshape_pred``
(src/models/components/liif.py:59-127,142-146) on given features with autograd on -- the decoder's part of the training path
sr_module.py:127-129 -> forward(lr, size, None) -- for synthetic ``imnet`` weights / features regenerated from ``synth.py``,
with the scalar loss  sum(out * R)  (R from synth.py, so d loss / d out = R), in fp32 and once more in float64.

float64: the reference LIIF does not run in float64 as it is (``make_coord`` ends in ``.float()`` and grid_sample rejects
the dtype mix), so ``make_coord`` is wrapped ON THE INSTANCE to cast its result to double; with that the ``.double()``
module runs.

The ReLU kink: the HIP kernels' summation order differs from ATen's, so a pre-activation ``a`` of imnet.layers.{0,2,4,6} within a
few ulp of 0 could flip a mask (6.9 million pre-activations at B = 2, 12x10 -> 31x27: no seed keeps all of them clear of zero, and
one flipped mask moves a gradient by per cent of its maximum).  So the cases are SMALL: ``a`` is taken with forward hooks on the
four hidden layers (four ensemble members each); seeds are tried from 123 upwards and the first with min|a| >= 2e-6 * gain over
all layers and members is kept (asserted; seed and minimum are stored).  A condition on the inputs, not a tolerance.

Stored per case, in a file of its own (liif_golden_grad_<case>.npz, each below 1 MiB):
  meta                      [b, h, w, hu, wu, gain, seed]
  min_abs_a                 min|a| over every virtual pixel, layer and hidden channel
  out                       fp32 output
  grad/feat                 fp32 d loss / d features
  grad/<imnet parameter>    fp32 d loss / d parameter; layers.0.weight at every 8th row (all columns)
  d64/<out|feat|parameter>  [max|fp32 - float64|, max|float64|] over the FULL tensor: the reference's own fp32 noise
Inputs are never stored.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_liif_grad.py
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
from src.models.components.liif import LIIF  # noqa: E402  (the reference)

# (name, B, H, W, Hu, Wu, gain)
CASES = [
    ("b2_3x2_5x4", 2, 3, 2, 5, 4, 1.0),                  # two images; 160 virtual pixels = 5 plane tiles
    ("b1_4x3_9x7", 1, 4, 3, 9, 7, 1.0),                  # non-integer scale on both axes; 252 virtual pixels: ragged last tile
    ("b1_8x8_5x6_down", 1, 8, 8, 5, 6, 1.0),             # down-scaling: most cells own no virtual pixel
    ("b1_1x1_7x5", 1, 1, 1, 7, 5, 1.0),                  # one cell: every shift clamps
    ("b1_2x3_8x12_gain2", 1, 2, 3, 8, 12, 2.0),          # exact x4: the +1e-6 decides the cell
]
ROW_STRIDE = 8
FIRST_SEED = 123
MIN_ABS_A = 2e-6                                         # x gain
HIDDEN_LAYERS = (0, 2, 4, 6)
IMNET_SHAPES = {"imnet.layers.0.weight": (256, 580), "imnet.layers.0.bias": (256,),
                **{f"imnet.layers.{i}.weight": (256, 256) for i in (2, 4, 6)}, **{f"imnet.layers.{i}.bias": (256,) for i in (2, 4, 6)},
                "imnet.layers.8.weight": (3, 256), "imnet.layers.8.bias": (3,)}


def inputs(seed, name, b, h, w, hu, wu, gain):
    sd = synth.state_dict_for(IMNET_SHAPES, seed, "liif.", gain=gain)
    feat = synth.encoder_features(seed, b, h, w)
    r = synth.uniform(seed, f"gradw:liif:{name}", (b, 3, hu, wu), 1.0)
    return sd, feat, r


def run(model, sd, feat, r, size, dtype):
    model.load_state_dict({k: torch.from_numpy(v).to(dtype) for k, v in sd.items()}, strict=False)
    model.zero_grad(set_to_none=True)
    seen = []
    hooks = [model.imnet.layers[i].register_forward_hook(lambda mod, args, res: seen.append(float(res.detach().abs().min())))
             for i in HIDDEN_LAYERS]
    x = torch.from_numpy(feat).to(dtype).requires_grad_(True)
    coord, cell = model.make_coord_and_cell(x, size)
    y = model.reshape_pred(model.query_rgb(x, coord, cell), size)
    for hook in hooks:
        hook.remove()
    assert len(seen) == 16                                       # four hidden layers x four ensemble members
    (y * torch.from_numpy(r).to(dtype)).sum().backward()
    grads = {k[len("imnet."):]: p.grad.numpy() for k, p in model.named_parameters() if k.startswith("imnet.")}
    return y.detach().numpy(), x.grad.numpy(), grads, min(seen)


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    m32 = LIIF().train()
    m64 = LIIF().double().train()
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
            out[f"grad/{pname}"] = (g[::ROW_STRIDE] if pname == "layers.0.weight" else g).astype(np.float32)
        worst = max(out[f"d64/{p}"][0] / max(out[f"d64/{p}"][1], 1e-30) for p in list(g32) + ["feat"])
        print(name, "seed", seed, "min|a| = %.3e" % min_a, "max|dfeat|=%.4f" % float(np.abs(f32).max()), "worst fp32-vs-f64 %.2e" % worst)
        path = os.path.join(HERE, f"liif_golden_grad_{name}.npz")
        np.savez_compressed(path, **out)
        print("wrote", path, os.path.getsize(path))


if __name__ == "__main__":
    main()
