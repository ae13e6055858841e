#!/usr/bin/env python3
"""Generate gradient fixtures for decoder modes 1 and 2 from the REAL reference decoder under autograd.

Build container only (needs /root/reference, read-only).  Runs the reference
``ImplicitDecoder(mode=m).forward(x, size, None)``, m in {1, 2}, with autograd on -- the training path of
sr_module.py:127-129 -- for synthetic weights/features regenerated from ``synth.py``, with the scalar
loss  sum(out * R)  (R from synth.py, so d loss / d out = R), in fp32 and once more in float64 (the same
module after ``.double()``: the truth, as make_golden_r8.py took it for the outputs).

Stored per case, in a file of its own (diinn_golden_grad_m12_<case>.npz; four files so that each stays below
the 1 MiB a committed file may have -- and below diinn_golden_grad.npz):
  meta                      [b, h, w, hu, wu, gain]
  out/m{m}                  fp32 output
  grad/m{m}/feat            fp32 d loss / d features
  grad/m{m}/<parameter>     fp32 d loss / d parameter; the K and Q WEIGHTS at every 8th output row (all columns)
  d64/m{m}/<out|feat|parameter>   [max|fp32 - float64|, max|float64|] over the FULL tensor: the reference's own fp32 noise
Inputs are never stored.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_grad_m12.py
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
    ("b2_12x10_31x27", 2, 12, 10, 31, 27, 1.0),          # 1674 pixels, 240 cells: both last tiles ragged
    ("b1_9x14_36x56_stress", 1, 9, 14, 36, 56, 3.0),     # the stress case of the mode-3 file
    ("b1_8x8_5x6_down", 1, 8, 8, 5, 6, 1.0),             # down-scaling: most cells own no pixel
    ("b1_1x1_7x5", 1, 1, 1, 7, 5, 1.0),                  # one cell
]
MODES = (1, 2)
ROW_STRIDE = 8


def strided(pname):
    return pname[0] in "KQ" and pname.endswith("weight")


def run(mode, sd, feat, r, size, dtype):
    dec = ImplicitDecoder(mode=mode, init_q=False)
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
        out = {"meta": np.array([b, h, w, hu, wu, gain], dtype=np.float64)}
        for m in MODES:
            sd = synth.decoder_state_dict(seed=123, gain=gain, mode=m)
            feat = synth.encoder_features(123, b, h, w)
            r = synth.uniform(123, f"gradw:m{m}:{name}", (b, 3, hu, wu), 1.0)
            y32, f32, g32 = run(m, sd, feat, r, (hu, wu), torch.float32)
            y64, f64, g64 = run(m, sd, feat, r, (hu, wu), torch.float64)

            def noise(a32, a64):
                return np.array([np.abs(a32.astype(np.float64) - a64).max(), np.abs(a64).max()], dtype=np.float64)

            out[f"out/m{m}"] = y32.astype(np.float32)
            out[f"d64/m{m}/out"] = noise(y32, y64)
            out[f"grad/m{m}/feat"] = f32.astype(np.float32)
            out[f"d64/m{m}/feat"] = noise(f32, f64)
            for pname, g in g32.items():
                out[f"d64/m{m}/{pname}"] = noise(g, g64[pname])
                out[f"grad/m{m}/{pname}"] = (g[::ROW_STRIDE] if strided(pname) else g).astype(np.float32)
            worst = max(out[f"d64/m{m}/{p}"][0] / max(out[f"d64/m{m}/{p}"][1], 1e-30) for p in g32)
            print(name, f"mode {m}", "max|dfeat|=%.4f" % float(np.abs(f32).max()), "worst fp32-vs-f64 %.2e" % worst)
        path = os.path.join(HERE, f"diinn_golden_grad_m12_{name}.npz")
        np.savez_compressed(path, **out)
        print("wrote", path, os.path.getsize(path))


if __name__ == "__main__":
    main()
